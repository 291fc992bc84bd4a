"""GPU suite: mi_denoise's median -- --modes median, --animation --animation-filter median (alone and as two frame blocks),
--median-radius, --median-plain -- on tiny frames: PNG frames with .png layers, EXR frames with .exr layers (FLOAT, and HALF with
--half).  Every output file holds the bits of Context.median_filter on the arrays the files decode to; the run prints its `median
radius <r> layers <n>` line and the `layer <file> sigma <value>` lines; the refusals that need a device write nothing; --modes all
lists no median file."""
import os
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import median_inputs as mi
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
N, SHAPE = 3, (20, 70)
LAYERS = ("albedo", "normal")                       # two render elements per frame, in sorted order
SIGMAS = (0.02, 0.1)


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _make(root, kind, half=False):
    d = root / "Animations" / "T"
    (d / "RenderElements").mkdir(parents=True)
    for i in range(N):
        noisy, g0, _ = mi.scene(SHAPE[0], SHAPE[1], seed=60 + i)
        layers, _ = mi.layer_set(g0, 2)
        if kind == "png":
            mid.save_image(d / f"Animation01_X_{i:04d}.png", mi.as_dtype(np.clip(noisy, 0, 1), np.uint8))
            for name, lyr in zip(LAYERS, layers):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.png", lyr)
        else:
            mid.save_image(d / f"Animation01_X_{i:04d}.exr", noisy)
            for name, lyr in zip(LAYERS, layers):
                f = lyr.astype(np.float32) / np.float32(255)
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.exr", f.astype(np.float16) if half else f)
    return d


def _decoded(d, kind, half):
    as_dt = np.float16 if half else None             # (load_image: None = a .png as uint8, an .exr as float32)
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.{kind}", as_dt) for i in range(N)]
    layers = [[mid.load_image(d / "RenderElements" / f"{name}_{i:04d}.{kind}", as_dt) for name in LAYERS] for i in range(N)]
    return frames, layers


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _lines(r):
    return [ln.strip() for ln in r.stdout.splitlines()]


@pytest.mark.parametrize("kind,half", [("png", False), ("exr", False), ("exr", True)], ids=["png", "exr-float", "exr-half"])
def test_median_modes_write_the_python_calls_bits(tmp_path, ctx, kind, half):
    d = _make(tmp_path, kind, half)
    frames, layers = _decoded(d, kind, half)
    out_dt = np.uint8 if kind == "png" else np.float16 if half else np.float32
    load_as = np.float16 if half else None
    common = ["--gpu-only"] + (["--half"] if half else [])

    # 1. one image, weighted by its two layers with one sigma each
    out = tmp_path / "o"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0001.{kind}", "--modes", "median", "--median-radius", 2, "--sigma-layers", "0.02,0.1", "--outdir", out] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(out) == [f"output-nonlinear-median.{kind}"]
    lines = _lines(r)
    assert "median radius 2 layers 2" in lines, r.stdout
    for name, sg in zip(LAYERS, SIGMAS):
        assert any(ln.startswith("layer ") and ln.endswith(f"{name}_0001.{kind} sigma {sg:g}") for ln in lines), r.stdout
    want = ctx.median_filter(frames[1], layers[1], SIGMAS, 2, out_dtype=out_dt)
    got = mid.load_image(out / f"output-nonlinear-median.{kind}", load_as)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))

    # 2. the animation with the defaults (radius 1, --sigma-c for every layer); --temporal-k is ignored
    out2 = tmp_path / "a"
    out2.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "median", "--sigma-c", 0.05, "--temporal-k", 2,
                        "--outdir", out2] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(out2))
    assert names == [f"output-animation-nonlinear-median-Animation01_X_{i:04d}.{kind}" for i in range(N)], names
    assert "median radius 1 layers 2" in _lines(r), r.stdout
    assert any(ln.startswith("layer ") and ln.endswith(f"albedo_0000.{kind} sigma 0.05") for ln in _lines(r)), r.stdout
    for i in range(N):
        want = ctx.median_filter(frames[i], layers[i], (0.05, 0.05), out_dtype=out_dt)
        got = mid.load_image(out2 / names[i], load_as)
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), i

    # 3. --median-plain loads no layer; two frame blocks on one device give the same files
    out3 = tmp_path / "o3"
    out3.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "median", "--gpus", 2, "--share-device",
                        "--median-radius", 3, "--median-plain", "--outdir", out3] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "median radius 3 layers 0" in _lines(r) and not any(ln.startswith("layer ") for ln in _lines(r)), r.stdout
    for i in range(N):
        want = ctx.median_filter(frames[i], radius=3, out_dtype=out_dt)
        got = mid.load_image(out3 / f"output-animation-nonlinear-median-Animation01_X_{i:04d}.{kind}", load_as)
        assert np.array_equal(_bits(got), _bits(want)), i
    out4 = tmp_path / "o4"
    out4.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0002.{kind}", "--modes", "median", "--median-plain", "--outdir", out4] + common)
    assert r.returncode == 0 and "median radius 1 layers 0" in _lines(r), r.stdout + r.stderr
    want = ctx.median_filter(frames[2], out_dtype=out_dt)
    assert np.array_equal(_bits(mid.load_image(out4 / f"output-nonlinear-median.{kind}", load_as)), _bits(want))


def test_refusals_that_need_a_device_write_nothing(tmp_path):
    d = _make(tmp_path, "png")
    os.remove(d / "RenderElements" / "normal_0002.png")                         # frame 2 has one layer, the others two
    n = 0

    def refused(target, args, *needles):
        nonlocal n
        out = tmp_path / f"r{n}"
        n += 1
        out.mkdir()
        r = _run(tmp_path, [d / target, "--gpu-only", "--outdir", out] + args)
        text = r.stdout + r.stderr
        assert r.returncode != 0 and all(x in text for x in needles), text
        assert os.listdir(out) == []

    refused("Animation01_X_0001.png", ["--modes", "median", "--sigma-layers", "0.1"], "--sigma-layers gives 1 sigma(s), but 2 layer file(s)")
    refused("Animation01_X_0000.png", ["--animation", "--animation-filter", "median"], "1 layer file(s), but", "every frame needs the same layers")
    refused("Animation01_X_0000.png", ["--animation", "--animation-filter", "median", "--halo", "rccl"], "--halo rccl is not available with --animation-filter median")
    for f in os.listdir(d / "RenderElements"):
        os.remove(d / "RenderElements" / f)
    refused("Animation01_X_0001.png", ["--modes", "median"], "0 layer file(s) found", "--median-plain")


def test_modes_all_lists_no_median_file(tmp_path):
    d = _make(tmp_path, "png")
    out = tmp_path / "all"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0001.png", "--gpu-only", "--radius", 4, "--outdir", out])      # --modes all is the default
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(f"output-{m}.png" for m in (
        "nonlinear-bialteral", "nonlinear-bialteral-layers", "linear-bialteral", "nonlinear-nlm", "nonlinear-nlm-multiframe",
        "nonlinear-nlm-multiframe-overlap"))
