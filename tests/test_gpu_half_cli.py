"""GPU suite: mi_denoise --half on HALF EXR frames -- the six GPU modes (single frame) and --animation --temporal-k 2.

With --half the frames are loaded as RGBA16F (mid_image_load_f16) and filtered as such; outputs are HALF EXR.  Since a half frame
filters to the bits of its widened RGBA32F frame, every output pixel must be numpy.float16 of the same run without --half, which
loads the same files as RGBA32F."""
import os
import struct
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from conftest import ROOT, synth_hdr, synth_ldr

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
H, W, N_FRAMES, TARGET = 96, 160, 5, 2
NAMES = ["output-nonlinear-bialteral", "output-nonlinear-bialteral-layers", "output-linear-bialteral",
         "output-nonlinear-nlm", "output-nonlinear-nlm-multiframe", "output-nonlinear-nlm-multiframe-overlap"]


def _make(root):
    rng = np.random.default_rng(61)
    d = root / "Anim"
    (d / "RenderElements").mkdir(parents=True)
    base = synth_hdr(rng, H, W, 2.0) * 0.25
    for i in range(N_FRAMES):
        f = (np.roll(base, 2 * i, axis=1) * rng.gamma(16.0, 1 / 16.0, (H, W, 1))).astype(np.float16)
        f[..., 3] = 1.0
        mid.save_image(d / f"Animation01_X_{i:04d}.exr", f)
    for name in ("albedo", "normal"):
        mid.save_image(d / "RenderElements" / f"{name}_{TARGET:04d}.png", synth_ldr(rng, H, W))
    return d


def _is_half_exr(path):
    blob = path.read_bytes()
    pos = blob.index(b"chlist\0") + 7 + 4
    types = []
    for _ in range(4):
        types.append(struct.unpack("<i", blob[pos + 2:pos + 6])[0])
        pos += 2 + 16
    return types == [1, 1, 1, 1]


def _run(tmp_path, d, out, args):
    out.mkdir()
    r = subprocess.run([CLI, str(d / f"Animation01_X_{TARGET:04d}.exr"), "--outdir", str(out)] + args, cwd=tmp_path,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_half_single_frame_modes(tmp_path):
    d = _make(tmp_path)
    _run(tmp_path, d, tmp_path / "f32", ["--gpu-only"])
    _run(tmp_path, d, tmp_path / "f16", ["--gpu-only", "--half"])
    assert sorted(os.listdir(tmp_path / "f16")) == sorted(f"{n}.exr" for n in NAMES)
    for n in NAMES:
        p16 = tmp_path / "f16" / f"{n}.exr"
        assert _is_half_exr(p16), n
        want = mid.load_image(tmp_path / "f32" / f"{n}.exr").astype(np.float16)
        assert np.array_equal(mid.load_image(p16, np.float16).view(np.uint16), want.view(np.uint16)), n


def test_half_animation(tmp_path):
    d = _make(tmp_path)
    _run(tmp_path, d, tmp_path / "f32", ["--animation", "--temporal-k", "2"])
    r = _run(tmp_path, d, tmp_path / "f16", ["--animation", "--temporal-k", "2", "--half"])
    assert "encoding png" not in r.stdout
    for i in range(N_FRAMES):
        name = f"output-animation-Animation01_X_{i:04d}.exr"
        p16 = tmp_path / "f16" / name
        assert _is_half_exr(p16), name
        want = mid.load_image(tmp_path / "f32" / name).astype(np.float16)
        assert np.array_equal(mid.load_image(p16, np.float16).view(np.uint16), want.view(np.uint16)), name
