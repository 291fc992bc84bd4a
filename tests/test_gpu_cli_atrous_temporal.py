"""GPU suite: mi_denoise --animation --animation-filter atrous-temporal on tiny frames -- a 4-frame PNG animation with .png layers
and a 3-frame EXR animation with .exr layers, 70 x 21, two layers, K = 1, three passes.  Every output file holds the bits of
Context.atrous_joint_temporal on the arrays the files decode to, alone and as two frame blocks with their halo frames; --halo
rccl and a --sigma-layers count other than the layer count are refused with nothing written; --animation-filter atrous keeps
ignoring --temporal-k; the help text lists the mode."""
import os
import subprocess

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
from conftest import ROOT
from test_gpu_kernel_bits import frame, guide

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
SHAPE = (21, 70)
COUNT = {"png": 4, "exr": 3}
LAYERS = ("albedo", "normal")                       # (sorted: the order the CLI finds them in)
SIGMAS = {"png": [0.15, 0.3], "exr": [0.5, 0.25]}
INFIX = "output-animation-nonlinear-atrous-multiframe-"


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _make(root, kind):
    """Frames and, under the discovery naming of the other CLI tests, one layer file per frame and layer name."""
    n = COUNT[kind]
    d = root / "Animations" / "T"
    (d / "RenderElements").mkdir(parents=True)
    if kind == "png":
        for i in range(n):
            mid.save_image(d / f"Animation01_X_{i:04d}.png", frame(SHAPE, i, i == 1, np.uint8))
            for l, name in enumerate(LAYERS):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.png", guide(SHAPE, i, l))
    else:
        for i, f in enumerate(gi.hdr_frames(SHAPE, n, seed=51)):
            mid.save_image(d / f"Animation01_X_{i:04d}.exr", f)
        rendered = gi.render_layers(SHAPE, n, np.float32, seed=52)
        for i in range(n):
            for name, lyr in zip(LAYERS, (rendered[i][1], rendered[i][0])):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.exr", lyr)
    return d


def _decoded(d, kind):
    n = COUNT[kind]
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.{kind}", None) for i in range(n)]
    layers = [[mid.load_image(d / "RenderElements" / f"{name}_{i:04d}.{kind}", None) for name in LAYERS] for i in range(n)]
    return frames, layers


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("kind", ["png", "exr"])
def test_atrous_temporal_writes_the_python_calls_bits(tmp_path, ctx, kind):
    d = _make(tmp_path, kind)
    n = COUNT[kind]
    frames, layers = _decoded(d, kind)
    sig = SIGMAS[kind]
    out_dt = np.uint8 if kind == "png" else np.float32
    mode = [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-temporal", "--temporal-k", 1, "--passes", 3,
            "--gpu-only", "--sigma-layers", ",".join(str(s) for s in sig)]
    want = ctx.atrous_joint_temporal(frames, layers, sig, k=1, passes=3, out_dtype=out_dt)
    assert not np.array_equal(_bits(want[1]), _bits(ctx.atrous_joint(frames[1], layers[1], sig, passes=3, out_dtype=out_dt)))   # the neighbours count
    for sub, more in (("a", []), ("b", ["--gpus", 2, "--share-device"])):          # alone; two frame blocks with their halo frames
        out = tmp_path / sub
        out.mkdir()
        r = _run(tmp_path, mode + ["--outdir", out] + more)
        assert r.returncode == 0, r.stdout + r.stderr
        names = sorted(os.listdir(out))
        assert names == [f"{INFIX}Animation01_X_{i:04d}.{kind}" for i in range(n)], names
        for i in range(n):
            got = mid.load_image(out / names[i], None)
            assert got.dtype == want[i].dtype and np.array_equal(_bits(got), _bits(want[i])), (sub, i)
    for name, s in zip(LAYERS, sig):                                               # the banner: one line per layer, in sorted order
        assert any(ln.strip().startswith("layer ") and f"{name}_0000.{kind} sigma {s:g}" in ln for ln in r.stdout.splitlines()), r.stdout

    # --temporal-k defaults to 2, the colour term joins with --atrous-sigma-color, five passes by default
    out = tmp_path / "c"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-temporal", "--gpu-only", "--sigma-c", 0.4,
                        "--atrous-sigma-color", 0.75, "--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    want = ctx.atrous_joint_temporal(frames, layers, [0.4, 0.4], k=2, color_sigma=0.75, out_dtype=out_dt)
    for i in range(n):
        got = mid.load_image(out / f"{INFIX}Animation01_X_{i:04d}.{kind}", None)
        assert np.array_equal(_bits(got), _bits(want[i])), i

    # --animation-filter atrous still ignores --temporal-k
    out = tmp_path / "d"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous", "--temporal-k", 2, "--passes", 3, "--gpu-only",
                        "--sigma-layers", ",".join(str(s) for s in sig), "--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == [f"output-animation-nonlinear-atrous-Animation01_X_{i:04d}.{kind}" for i in range(n)]
    for i in range(n):
        got = mid.load_image(out / f"output-animation-nonlinear-atrous-Animation01_X_{i:04d}.{kind}", None)
        assert np.array_equal(_bits(got), _bits(ctx.atrous_joint(frames[i], layers[i], sig, passes=3, out_dtype=out_dt))), i


def test_refusals_write_nothing_and_help_lists_the_mode(tmp_path):
    d = _make(tmp_path, "exr")
    anim = [d / "Animation01_X_0000.exr", "--animation", "--animation-filter", "atrous-temporal", "--gpu-only"]
    for j, (args, needles) in enumerate(((["--halo", "rccl"], ["--halo rccl is not available with --animation-filter atrous-temporal"]),
                                         (["--sigma-layers", "0.5,0.25,0.1"], ["--sigma-layers", "3 sigma", "2 layer"]))):
        out = tmp_path / f"r{j}"
        out.mkdir()
        r = _run(tmp_path, anim + ["--outdir", out] + args)
        text = r.stdout + r.stderr
        assert r.returncode != 0 and all(x in text for x in needles), text
        assert os.listdir(out) == []
    h = _run(tmp_path, ["--help"]).stdout
    assert "or atrous-temporal:" in h and "output-animation-nonlinear-atrous-multiframe-*" in h
