"""GPU suite: mi_denoise --animation --animation-filter bilateral | linear | layers -- the bilateral of every frame of a small
synthetic animation, each frame guided by its own RenderElements layers in the `layers` mode.  Every output file must hold the
Python per-frame call (ctx.bilateral / ctx.bilateral_layers) in the file's format: the reference's u8 read-back conversion for
PNG, RGBA16F rounding for --half, RGBA32F for EXR."""
import os
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from conftest import ROOT
from test_cli import _make_animation

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
N = 5
PREFIX = {"bilateral": "output-animation-nonlinear-bialteral-", "linear": "output-animation-linear-bialteral-",
          "layers": "output-animation-nonlinear-bialteral-layers-"}


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _want(ctx, frame, layers, mode, r, kind):
    if mode == "layers":
        f32 = ctx.bilateral_layers(frame, layers, r, 2.0, 0.2)
    else:
        f32 = ctx.bilateral(frame, r, 2.0, 0.2, "linear" if mode == "linear" else "texture")
    return ctx.pack_u8(f32) if kind == "png" else ctx.pack_f16(f32) if kind == "half" else f32


@pytest.mark.parametrize("kind", ["png", "exr", "half"])
def test_animation_filters_write_the_per_frame_results(tmp_path, ctx, kind):
    d, _, layers, ext = _make_animation(tmp_path, kind != "png", n=N)
    target = d / f"Animation01_X_0000.{ext}"
    for mode in ("bilateral", "linear", "layers"):
        out = tmp_path / f"o_{mode}"
        out.mkdir()
        extra = ["--half"] if kind == "half" else []
        r = _run(tmp_path, [target, "--animation", "--animation-filter", mode, "--radius", 8, "--outdir", out] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        names = sorted(os.listdir(out))
        out_ext = "png" if kind == "png" else "exr"
        assert names == [f"{PREFIX[mode]}Animation01_X_{i:04d}.{out_ext}" for i in range(N)], names
        for i in range(N):
            # the frame as the CLI reads it: PNG as RGBA8, EXR as RGBA32F, --half EXR as RGBA16F
            frame = mid.load_image(d / f"Animation01_X_{i:04d}.{ext}", np.float16 if kind == "half" else None)
            want = _want(ctx, frame, layers[i], mode, 8, kind)
            got = mid.load_image(out / names[i], np.float16 if kind == "half" else None)
            assert got.dtype == want.dtype and got.shape == want.shape, (mode, i)
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (mode, i)
        # frame blocks over three (rehearsed) devices give the same bytes
        out3 = tmp_path / f"o3_{mode}"
        out3.mkdir()
        r = _run(tmp_path, [target, "--animation", "--animation-filter", mode, "--radius", 8, "--outdir", out3,
                            "--gpus", 3, "--share-device"] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        for n in names:
            assert (out3 / n).read_bytes() == (out / n).read_bytes(), (mode, n)


def test_missing_layer_and_rccl_halo_are_refused(tmp_path):
    d, _, _, ext = _make_animation(tmp_path, False, n=N)
    target = d / "Animation01_X_0000.png"
    out = tmp_path / "o"
    out.mkdir()
    r = _run(tmp_path, [target, "--animation", "--animation-filter", "bilateral", "--halo", "rccl", "--outdir", out])
    assert r.returncode != 0 and "--halo rccl" in r.stdout + r.stderr
    os.remove(d / "RenderElements" / "normal_0003.png")
    r = _run(tmp_path, [target, "--animation", "--animation-filter", "layers", "--outdir", out])
    assert r.returncode != 0 and "Animation01_X_0003" in r.stdout + r.stderr, r.stdout + r.stderr
    assert os.listdir(out) == []


def test_default_animation_filter_keeps_its_names(tmp_path):
    d, _, _, ext = _make_animation(tmp_path, False, n=N)
    target = d / "Animation01_X_0000.png"
    outs = []
    for extra in ([], ["--animation-filter", "nlm"]):
        out = tmp_path / f"o{len(outs)}"
        out.mkdir()
        r = _run(tmp_path, [target, "--animation", "--temporal-k", 1, "--outdir", out] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "temporal nonlocal" in r.stdout
        assert sorted(os.listdir(out)) == [f"output-animation-Animation01_X_{i:04d}.png" for i in range(N)]
        outs.append(out)
    for i in range(N):
        name = f"output-animation-Animation01_X_{i:04d}.png"
        assert (outs[0] / name).read_bytes() == (outs[1] / name).read_bytes()
