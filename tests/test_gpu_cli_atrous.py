"""GPU suite: mi_denoise's a-trous modes -- --modes atrous, --animation --animation-filter atrous (alone and as two frame blocks),
--passes, --sigma-layers, --atrous-sigma-color -- on tiny frames: PNG frames with .png layers, EXR frames with .exr layers (FLOAT,
and HALF with --half).  Every output file holds the bits of Context.atrous_joint on the arrays the files decode to; a
--sigma-layers count other than the layer count, --passes 0 and 9, mixed .png / .exr layers and --halo rccl are refused with
nothing written; --modes all lists no atrous file."""
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
N, SHAPE = 3, (20, 70)
LAYERS = ("albedo", "normal")                       # (sorted: the order the CLI finds them in)
SIGMAS = {"png": [0.15, 0.3], "exr": [0.5, 0.25]}


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _make(root, kind, half=False):
    """Frames and, under the discovery naming of the other CLI tests, one layer file per frame and layer name."""
    d = root / "Animations" / "T"
    (d / "RenderElements").mkdir(parents=True)
    if kind == "png":
        for i in range(N):
            mid.save_image(d / f"Animation01_X_{i:04d}.png", frame(SHAPE, i, i == 1, np.uint8))
            for l, name in enumerate(LAYERS):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.png", guide(SHAPE, i, l))
    else:
        for i, f in enumerate(gi.hdr_frames(SHAPE, N, seed=51)):
            mid.save_image(d / f"Animation01_X_{i:04d}.exr", f)
        rendered = gi.render_layers(SHAPE, N, np.float16 if half else np.float32, seed=52)
        for i in range(N):
            for name, lyr in zip(LAYERS, (rendered[i][1], rendered[i][0])):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.exr", lyr)
    return d


def _decoded(d, kind, half):
    as_dt = np.float16 if half else None             # (load_image: None = a .png as uint8, an .exr as float32)
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.{kind}", as_dt) for i in range(N)]
    layers = [[mid.load_image(d / "RenderElements" / f"{name}_{i:04d}.{kind}", as_dt) for name in LAYERS] for i in range(N)]
    return frames, layers


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("kind,half", [("png", False), ("exr", False), ("exr", True)], ids=["png", "exr-float", "exr-half"])
def test_atrous_modes_write_the_python_calls_bits(tmp_path, ctx, kind, half):
    d = _make(tmp_path, kind, half)
    frames, layers = _decoded(d, kind, half)
    sig = SIGMAS[kind]
    out_dt = np.uint8 if kind == "png" else np.float16 if half else np.float32
    load_as = np.float16 if half else None
    common = ["--gpu-only", "--sigma-layers", ",".join(str(s) for s in sig)] + (["--half"] if half else [])

    # 1. one image, three passes with the colour term
    out = tmp_path / "o"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0001.{kind}", "--modes", "atrous", "--passes", 3, "--atrous-sigma-color", 0.75, "--outdir", out] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(out) == [f"output-nonlinear-atrous.{kind}"]
    for name, s in zip(LAYERS, sig):                                               # the banner: one line per layer, in sorted order
        assert any(ln.strip().startswith("layer ") and f"{name}_0001.{kind} sigma {s:g}" in ln for ln in r.stdout.splitlines()), r.stdout
    want = ctx.atrous_joint(frames[1], layers[1], sig, passes=3, color_sigma=0.75)
    want = ctx.pack_u8(want) if kind == "png" else ctx.pack_f16(want) if half else want
    got = mid.load_image(out / f"output-nonlinear-atrous.{kind}", load_as)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))

    # 2. the animation, five passes by default; --temporal-k is ignored
    out2 = tmp_path / "a"
    out2.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous", "--temporal-k", 2, "--outdir", out2] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(out2))
    assert names == [f"output-animation-nonlinear-atrous-Animation01_X_{i:04d}.{kind}" for i in range(N)], names
    want = [ctx.atrous_joint(f, ls, sig, out_dtype=out_dt) for f, ls in zip(frames, layers)]
    for i in range(N):
        got = mid.load_image(out2 / names[i], load_as)
        assert got.dtype == want[i].dtype and np.array_equal(_bits(got), _bits(want[i])), i

    # 3. without --sigma-layers: --sigma-c in every layer; two frame blocks on one device give the same files
    out3 = tmp_path / "o3"
    out3.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous", "--gpus", 2, "--share-device", "--gpu-only",
                        "--passes", 2, "--sigma-c", 0.4, "--outdir", out3] + (["--half"] if half else []))
    assert r.returncode == 0, r.stdout + r.stderr
    for i in range(N):
        want = ctx.atrous_joint(frames[i], layers[i], [0.4, 0.4], passes=2, out_dtype=out_dt)
        got = mid.load_image(out3 / f"output-animation-nonlinear-atrous-Animation01_X_{i:04d}.{kind}", load_as)
        assert np.array_equal(_bits(got), _bits(want)), i


def test_refusals_write_nothing(tmp_path):
    d = _make(tmp_path, "exr")
    single = ("Animation01_X_0001.exr", ["--modes", "atrous"])
    anim = ("Animation01_X_0000.exr", ["--animation", "--animation-filter", "atrous"])
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

    for target, mode in (single, anim):
        refused(target, mode + ["--sigma-layers", "0.5,0.25,0.1"], "--sigma-layers", "3 sigma", "2 layer")
        refused(target, mode + ["--passes", 0], "--passes 0", "1..8")
        refused(target, mode + ["--passes", 9], "--passes 9", "1..8")
    refused(anim[0], anim[1] + ["--halo", "rccl"], "--halo rccl is not available with --animation-filter atrous")
    os.remove(d / "RenderElements" / "normal_0001.exr")
    mid.save_image(d / "RenderElements" / "normal_0001.png", np.full(SHAPE + (4,), 128, np.uint8))
    for target, mode in (single, anim):
        refused(target, mode, "normal_0001.png", "one format")


def test_modes_all_lists_no_atrous_file_and_help_lists_the_options(tmp_path):
    d = _make(tmp_path, "png")
    out = tmp_path / "all"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0001.png", "--gpu-only", "--radius", 4, "--outdir", out])      # --modes all is the default
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(f"output-{m}.png" for m in (
        "nonlinear-bialteral", "nonlinear-bialteral-layers", "linear-bialteral", "nonlinear-nlm", "nonlinear-nlm-multiframe",
        "nonlinear-nlm-multiframe-overlap"))
    h = _run(tmp_path, ["--help"]).stdout
    assert "\n  --passes N " in h and "\n  --atrous-sigma-color X " in h
    assert "output-nonlinear-atrous.{png,exr}" in h and "output-animation-nonlinear-atrous-*" in h
