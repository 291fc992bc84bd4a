"""GPU suite: mi_denoise's variance-guided a-trous modes -- --modes atrous-variance and --animation --animation-filter atrous-variance
(alone and as two frame blocks with their halo frames), --passes, --sigma-layers, --atrous-sigma-lum, --atrous-epsilon, --temporal-k
-- on tiny frames: a 4-frame PNG animation with .png layers and a 3-frame EXR animation with .exr layers, 70 x 21, two layers.
Every output file holds the bits of Context.atrous_moments + Context.atrous_variance on the arrays the files decode to; --halo
rccl and a --sigma-layers count other than the layer count are refused with nothing written; the help text lists the modes."""
import os
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from test_gpu_cli_atrous_temporal import COUNT, LAYERS, SIGMAS, _bits, _decoded, _make

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image_denoising_filter_amd", "mi_denoise")
INFIX = "output-animation-nonlinear-atrous-variance-"


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _resident(ctx, frames, layers, sig, k, t, out_dt, **kw):
    return ctx.atrous_variance(frames[t], ctx.atrous_moments(frames, layers, sig, k=k, t=t), layers[t], sig, out_dtype=out_dt, **kw)


@pytest.mark.parametrize("kind", ["png", "exr"])
def test_atrous_variance_writes_the_python_calls_bits(tmp_path, ctx, kind):
    d = _make(tmp_path, kind)
    n = COUNT[kind]
    frames, layers = _decoded(d, kind)
    sig = SIGMAS[kind]
    out_dt = np.uint8 if kind == "png" else np.float32
    common = ["--gpu-only", "--sigma-layers", ",".join(str(s) for s in sig)]

    # 1. one image: the moments of the image alone (k = 0), then the passes
    out = tmp_path / "single"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0001.{kind}", "--modes", "atrous-variance", "--passes", 3, "--atrous-sigma-lum", 2, "--atrous-epsilon", 0.01,
                        "--outdir", out] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(out) == [f"output-nonlinear-atrous-variance.{kind}"]
    for name, s in zip(LAYERS, sig):                                               # the banner: one line per layer, in sorted order
        assert any(ln.strip().startswith("layer ") and f"{name}_0001.{kind} sigma {s:g}" in ln for ln in r.stdout.splitlines()), r.stdout
    want = _resident(ctx, frames[1:2], layers[1:2], sig, 0, 0, np.float32, passes=3, sigma_lum=2.0, epsilon=0.01)
    if kind == "png":
        want = ctx.pack_u8(want)                                                    # the single-image modes write the float result's read-back
    got = mid.load_image(out / f"output-nonlinear-atrous-variance.{kind}", None)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))

    # 2. the animation: --temporal-k is the window of the moments; alone, and as two frame blocks with their halo frames
    mode = [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-variance", "--temporal-k", 1, "--passes", 3] + common
    want = [_resident(ctx, frames, layers, sig, 1, t, out_dt, passes=3) for t in range(n)]
    assert not np.array_equal(_bits(want[1]), _bits(_resident(ctx, frames, layers, sig, 0, 1, out_dt, passes=3)))    # the neighbours count
    for sub, more in (("a", []), ("b", ["--gpus", 2, "--share-device"])):
        out = tmp_path / sub
        out.mkdir()
        r = _run(tmp_path, mode + ["--outdir", out] + more)
        assert r.returncode == 0, r.stdout + r.stderr
        names = sorted(os.listdir(out))
        assert names == [f"{INFIX}Animation01_X_{i:04d}.{kind}" for i in range(n)], names
        for i in range(n):
            got = mid.load_image(out / names[i], None)
            assert got.dtype == want[i].dtype and np.array_equal(_bits(got), _bits(want[i])), (sub, i)

    # 3. the defaults: K = 2, five passes, sigma_lum 4, epsilon 1e-3
    out = tmp_path / "c"
    out.mkdir()
    r = _run(tmp_path, [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-variance", "--gpu-only", "--sigma-c", 0.4, "--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    for i in range(n):
        got = mid.load_image(out / f"{INFIX}Animation01_X_{i:04d}.{kind}", None)
        want_i = _resident(ctx, frames, layers, [0.4, 0.4], 2, i, out_dt, passes=5, sigma_lum=4.0, epsilon=1e-3)
        assert np.array_equal(_bits(got), _bits(want_i)), i


def test_refusals_write_nothing_and_help_lists_the_modes(tmp_path):
    d = _make(tmp_path, "exr")
    anim = [d / "Animation01_X_0000.exr", "--animation", "--animation-filter", "atrous-variance", "--gpu-only"]
    for j, (args, needles) in enumerate(((["--halo", "rccl"], ["--halo rccl is not available with --animation-filter atrous-variance"]),
                                         (["--sigma-layers", "0.5,0.25,0.1"], ["--sigma-layers", "3 sigma", "2 layer"]),
                                         (["--atrous-epsilon", "0"], ["epsilon"]), (["--atrous-sigma-lum", "-1"], ["sigmaLum"]))):
        out = tmp_path / f"r{j}"
        out.mkdir()
        r = _run(tmp_path, anim + ["--outdir", out] + args)
        text = r.stdout + r.stderr
        assert r.returncode != 0 and all(x in text for x in needles), text
        assert os.listdir(out) == []
    h = _run(tmp_path, ["--help"]).stdout
    assert "and atrous-variance (not part of all)" in h and "output-nonlinear-atrous-variance.{png,exr}" in h
    assert "or atrous-variance:" in h and "output-animation-nonlinear-atrous-variance-*" in h
    assert "--atrous-sigma-lum X" in h and "--atrous-epsilon X" in h
