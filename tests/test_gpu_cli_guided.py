"""GPU suite: mi_denoise's guided filter -- --modes guided, --animation --animation-filter guided (alone and as two frame blocks),
--guided-radius, --guided-eps, --guide-layer -- on tiny frames: PNG frames with a .png guide, EXR frames with an .exr guide (FLOAT,
and HALF with --half), and frames that guide themselves.  Every output file holds the bits of Context.guided_filter on the arrays the
files decode to; the run prints its `guided guide <file|self> radius <r> eps <x>` line; a --guide-layer that matches no file or two
is refused by name with nothing written; --modes all lists no guided file."""
import os
import subprocess

import numpy as np
import pytest

import guided_inputs as gi
import image_denoising_filter_amd as mid
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
N, SHAPE = 3, (20, 70)
LAYERS = ("albedo", "normal")                       # two render elements per frame: --guide-layer picks one


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _make(root, kind, half=False):
    d = root / "Animations" / "T"
    (d / "RenderElements").mkdir(parents=True)
    for i in range(N):
        noisy, alb, _ = gi.scene(SHAPE[0], SHAPE[1], 2, seed=60 + i)
        other = gi.scene(SHAPE[0], SHAPE[1], 3, seed=70 + i)[1]
        if kind == "png":
            mid.save_image(d / f"Animation01_X_{i:04d}.png", gi.as_dtype(noisy, np.uint8))
            for name, lyr in zip(LAYERS, (alb, other)):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.png", gi.as_dtype(lyr, np.uint8))
        else:
            mid.save_image(d / f"Animation01_X_{i:04d}.exr", noisy * np.float32(3))
            for name, lyr in zip(LAYERS, (alb, other)):
                mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.exr", lyr.astype(np.float16) if half else lyr)
    return d


def _decoded(d, kind, half):
    as_dt = np.float16 if half else None             # (load_image: None = a .png as uint8, an .exr as float32)
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.{kind}", as_dt) for i in range(N)]
    guides = [mid.load_image(d / "RenderElements" / f"albedo_{i:04d}.{kind}", as_dt) for i in range(N)]
    return frames, guides


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("kind,half", [("png", False), ("exr", False), ("exr", True)], ids=["png", "exr-float", "exr-half"])
def test_guided_modes_write_the_python_calls_bits(tmp_path, ctx, kind, half):
    d = _make(tmp_path, kind, half)
    frames, guides = _decoded(d, kind, half)
    out_dt = np.uint8 if kind == "png" else np.float16 if half else np.float32
    load_as = np.float16 if half else None
    common = ["--gpu-only"] + (["--half"] if half else [])

    # 1. one image, guided by its albedo
    out = tmp_path / "o"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0001.{kind}", "--modes", "guided", "--guided-radius", 3, "--guided-eps", 0.001, "--guide-layer", "albedo",
                        "--outdir", out] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(out) == [f"output-nonlinear-guided.{kind}"]
    assert any(ln.strip().startswith("guided guide ") and ln.strip().endswith(f"albedo_0001.{kind} radius 3 eps 0.001") for ln in r.stdout.splitlines()), r.stdout
    want = ctx.guided_filter(frames[1], guides[1], 3, 1e-3)
    want = ctx.pack_u8(want) if kind == "png" else ctx.pack_f16(want) if half else want
    got = mid.load_image(out / f"output-nonlinear-guided.{kind}", load_as)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))

    # 2. the animation with the defaults (radius 8, eps 0.01); --temporal-k is ignored
    out2 = tmp_path / "a"
    out2.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "guided", "--guide-layer", "albedo", "--temporal-k", 2,
                        "--outdir", out2] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(out2))
    assert names == [f"output-animation-nonlinear-guided-Animation01_X_{i:04d}.{kind}" for i in range(N)], names
    assert any(ln.strip().startswith("guided guide ") and ln.strip().endswith(f"albedo_0000.{kind} radius 8 eps 0.01") for ln in r.stdout.splitlines()), r.stdout
    for i in range(N):
        want = ctx.guided_filter(frames[i], guides[i], out_dtype=out_dt)
        got = mid.load_image(out2 / names[i], load_as)
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), i

    # 3. without --guide-layer every frame guides itself and no layer is read; two frame blocks on one device give the same files
    out3 = tmp_path / "o3"
    out3.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "guided", "--gpus", 2, "--share-device",
                        "--guided-radius", 2, "--outdir", out3] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert any(ln.strip() == "guided guide self radius 2 eps 0.01" for ln in r.stdout.splitlines()), r.stdout
    for i in range(N):
        want = ctx.guided_filter(frames[i], None, 2, out_dtype=out_dt)
        got = mid.load_image(out3 / f"output-animation-nonlinear-guided-Animation01_X_{i:04d}.{kind}", load_as)
        assert np.array_equal(_bits(got), _bits(want)), i
    out4 = tmp_path / "o4"
    out4.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0002.{kind}", "--modes", "guided", "--outdir", out4] + common)
    assert r.returncode == 0 and any(ln.strip() == "guided guide self radius 8 eps 0.01" for ln in r.stdout.splitlines()), r.stdout + r.stderr
    want = ctx.guided_filter(frames[2], None, out_dtype=out_dt)
    assert np.array_equal(_bits(mid.load_image(out4 / f"output-nonlinear-guided.{kind}", load_as)), _bits(want))


def test_refusals_write_nothing(tmp_path):
    d = _make(tmp_path, "png")
    single = ("Animation01_X_0001.png", ["--modes", "guided"])
    anim = ("Animation01_X_0000.png", ["--animation", "--animation-filter", "guided"])
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
        refused(target, mode + ["--guide-layer", "depth"], "--guide-layer depth matches 0 layer file(s)", "exactly one")
        refused(target, mode + ["--guide-layer", "a"], "--guide-layer a matches 2 layer file(s)", "exactly one")      # albedo and normal
        refused(target, mode + ["--guided-radius", 0], "--guided-radius 0", "1..16")
        refused(target, mode + ["--guided-radius", 17], "--guided-radius 17", "1..16")
        refused(target, mode + ["--guided-eps", 0], "--guided-eps 0", "finite and > 0")
    refused(anim[0], anim[1] + ["--halo", "rccl"], "--halo rccl is not available with --animation-filter guided")
    refused(single[0], ["--modes", "atrous", "--guide-layer", "albedo"], "--guide-layer applies to --modes guided")
    refused(anim[0], ["--animation", "--animation-filter", "atrous", "--guided-eps", "0.1"], "--guided-eps applies to")


def test_modes_all_lists_no_guided_file_and_help_lists_the_options(tmp_path):
    d = _make(tmp_path, "png")
    out = tmp_path / "all"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0001.png", "--gpu-only", "--radius", 4, "--outdir", out])      # --modes all is the default
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(f"output-{m}.png" for m in (
        "nonlinear-bialteral", "nonlinear-bialteral-layers", "linear-bialteral", "nonlinear-nlm", "nonlinear-nlm-multiframe",
        "nonlinear-nlm-multiframe-overlap"))
    h = _run(tmp_path, ["--help"]).stdout
    assert "\n  --guided-radius R " in h and "\n  --guided-eps X " in h and "\n  --guide-layer SUBSTR " in h
    assert "output-nonlinear-guided.{png,exr}" in h and "output-animation-nonlinear-guided-*" in h
