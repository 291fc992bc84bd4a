"""GPU suite: mi_denoise --animation --animation-filter bilateral-temporal | layers-temporal (the bilateral of every frame over
the frames t-K..t+K, plain or guided by the frames' RenderElements layers): output names, the pixels of the Python call
(ctx.bilateral_temporal) in the file's format, frame blocks over two contexts give the same bytes, a missing layer is refused."""
import os
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from conftest import ROOT
from test_cli import _make_animation

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
N, H, W = 5, 45, 133
NAMES = {"bilateral-temporal": "nonlinear-bialteral-multiframe", "layers-temporal": "nonlinear-bialteral-layers-multiframe"}


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("value", list(NAMES))
def test_files_hold_the_python_calls_bits_and_blocks_give_the_same_bytes(tmp_path, ctx, value):
    d, _, layers, ext = _make_animation(tmp_path, False, n=N, h=H, w=W)
    target = d / "Animation01_X_0000.png"
    out = tmp_path / "o"
    out.mkdir()
    args = [target, "--animation", "--animation-filter", value, "--temporal-k", 1, "--radius", 8, "--sigma-s", 3.0, "--sigma-c", 0.15]
    r = _run(tmp_path, args + ["--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "multiframe" in r.stdout
    names = sorted(os.listdir(out))
    assert names == [f"output-animation-{NAMES[value]}-Animation01_X_{i:04d}.png" for i in range(N)], names
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.png") for i in range(N)]
    ll = [layers[i] for i in range(N)] if value == "layers-temporal" else None
    want = ctx.bilateral_temporal(frames, 1, radius=8, sigma_s=3.0, sigma_c=0.15, layers=ll, out_dtype=np.uint8)
    for i in range(N):
        got = mid.load_image(out / names[i])
        assert got.dtype == np.uint8 and np.array_equal(got, want[i]), i
    out2 = tmp_path / "o2"
    out2.mkdir()
    r = _run(tmp_path, args + ["--outdir", out2, "--gpus", 2, "--share-device"])
    assert r.returncode == 0, r.stdout + r.stderr
    for n in names:
        assert (out2 / n).read_bytes() == (out / n).read_bytes(), n


def test_a_missing_layer_is_refused_naming_the_frame(tmp_path):
    d, _, _, _ = _make_animation(tmp_path, False, n=N, h=H, w=W)
    out = tmp_path / "o"
    out.mkdir()
    os.remove(d / "RenderElements" / "normal_0003.png")
    r = _run(tmp_path, [d / "Animation01_X_0000.png", "--animation", "--animation-filter", "layers-temporal", "--outdir", out])
    assert r.returncode != 0 and "Animation01_X_0003" in r.stdout + r.stderr, r.stdout + r.stderr
    assert os.listdir(out) == []
