"""GPU suite: mi_denoise's joint NLM modes -- --modes nlm-joint, --animation --animation-filter nlm-joint / nlm-joint-temporal,
--h-layers -- on tiny PNG frames with two .png layers each.  Every output file holds the bits of Context.nlm_joint on the arrays the
files decode to; the run prints one `layer <file> h <value>` line per layer; an --h-layers count other than the layer count and an
.exr layer are refused; --modes all writes the files it always wrote."""
import os
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from conftest import ROOT
from test_gpu_kernel_bits import frame, guide

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
N, SHAPE = 3, (20, 70)
LAYERS = ("albedo", "normal")                       # (sorted: the order the CLI finds them in)
HS = [0.6, 0.9]


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _make(root):
    """Frames and, under the discovery naming of the other CLI tests, one layer file per frame and layer name."""
    d = root / "Animations" / "T"
    (d / "RenderElements").mkdir(parents=True)
    for i in range(N):
        mid.save_image(d / f"Animation01_X_{i:04d}.png", frame(SHAPE, i, i == 1, np.uint8))
        for l, name in enumerate(LAYERS):
            mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.png", guide(SHAPE, i, l))
    return d


def _decoded(d):
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.png") for i in range(N)]
    layers = [[mid.load_image(d / "RenderElements" / f"{name}_{i:04d}.png") for name in LAYERS] for i in range(N)]
    return frames, layers


@pytest.mark.parametrize("window", ["default", "21x21"])
def test_nlm_joint_modes_write_the_python_calls_bits(tmp_path, ctx, window):
    d = _make(tmp_path)
    frames, layers = _decoded(d)
    kw = dict(search=(-7, 7), patch=(-3, 3)) if window == "default" else dict(search=(-10, 11), patch=(-3, 4))
    common = ["--gpu-only", "--h-layers", ",".join(str(s) for s in HS)] + ([] if window == "default" else ["--search", "-10,11", "--patch", "-3,4"])

    out = tmp_path / "o"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0001.png", "--modes", "nlm-joint", "--outdir", out] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(out) == ["output-nonlinear-nlm-joint.png"]
    for name, s in zip(LAYERS, HS):                                                # the banner: one line per layer, in sorted order
        assert any(ln.strip().startswith("layer ") and f"{name}_0001.png h {s:g}" in ln for ln in r.stdout.splitlines()), r.stdout
    want = ctx.pack_u8(ctx.nlm_joint(frames[1:2], layers[1:2], HS, 0, **kw)[0])
    got = mid.load_image(out / "output-nonlinear-nlm-joint.png")
    assert got.dtype == want.dtype and np.array_equal(got, want)

    for value, k, stem, extra in (("nlm-joint", 0, "output-animation-nonlinear-nlm-joint-", ["--temporal-k", 2]),
                                  ("nlm-joint-temporal", 1, "output-animation-nonlinear-nlm-joint-multiframe-", ["--temporal-k", 1])):
        out2 = tmp_path / ("a-" + value)
        out2.mkdir()
        r = _run(tmp_path, [d / "Animation01_X_0000.png", "--animation", "--animation-filter", value, "--outdir", out2] + extra + common)
        assert r.returncode == 0, r.stdout + r.stderr
        for name, s in zip(LAYERS, HS):
            assert any(ln.strip().startswith("layer ") and f"{name}_0000.png h {s:g}" in ln for ln in r.stdout.splitlines()), r.stdout
        names = sorted(os.listdir(out2))
        assert names == [f"{stem}Animation01_X_{i:04d}.png" for i in range(N)], names
        want = ctx.nlm_joint(frames, layers, HS, k, out_dtype=np.uint8, **kw)
        for i in range(N):
            got = mid.load_image(out2 / names[i])
            assert got.dtype == want[i].dtype and np.array_equal(got, want[i]), (value, i)

    # without --h-layers: --nlm-h in every layer; two frame blocks on one device give the same files
    out3 = tmp_path / "o3"
    out3.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0000.png", "--animation", "--animation-filter", "nlm-joint-temporal", "--temporal-k", 1, "--gpus", 2,
                        "--share-device", "--gpu-only", "--nlm-h", 0.8, "--outdir", out3] + common[3:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sum("h 0.8" in ln for ln in r.stdout.splitlines() if ln.strip().startswith("layer ")) == len(LAYERS)
    want = ctx.nlm_joint(frames, layers, None, 1, hparam=0.8, out_dtype=np.uint8, **kw)
    for i in range(N):
        got = mid.load_image(out3 / f"output-animation-nonlinear-nlm-joint-multiframe-Animation01_X_{i:04d}.png")
        assert np.array_equal(got, want[i]), i


def test_h_count_mismatch_and_exr_layers_are_refused(tmp_path):
    d = _make(tmp_path)
    modes = (("Animation01_X_0001.png", ["--modes", "nlm-joint"]),
             ("Animation01_X_0000.png", ["--animation", "--animation-filter", "nlm-joint"]),
             ("Animation01_X_0000.png", ["--animation", "--animation-filter", "nlm-joint-temporal"]))
    for target, mode in modes:
        out = tmp_path / ("s" + mode[-1] + str(len(mode)))
        out.mkdir()
        r = _run(tmp_path, [d / target, "--gpu-only", "--h-layers", "0.5,0.25,0.1", "--outdir", out] + mode)
        text = r.stdout + r.stderr
        assert r.returncode != 0 and "--h-layers" in text and "3 value" in text and "2 layer" in text, text
        assert os.listdir(out) == []
    # an .exr layer: refused with the wording of the other NLM modes, whatever they say about it
    os.remove(d / "RenderElements" / "normal_0001.png")
    mid.save_image(d / "RenderElements" / "normal_0001.exr", np.full(SHAPE + (4,), 0.5, np.float32))
    ref = _run(tmp_path, [d / "Animation01_X_0001.png", "--gpu-only", "--modes", "nlm-layers", "--outdir", tmp_path])
    assert ref.returncode != 0 and "normal_0001.exr" in ref.stdout + ref.stderr
    wording = [ln for ln in (ref.stdout + ref.stderr).splitlines() if "normal_0001.exr" in ln][-1]
    for target, mode in modes:
        out = tmp_path / ("m" + mode[-1] + str(len(mode)))
        out.mkdir()
        r = _run(tmp_path, [d / target, "--gpu-only", "--outdir", out] + mode)
        assert r.returncode != 0 and wording in (r.stdout + r.stderr).splitlines(), r.stdout + r.stderr
        assert os.listdir(out) == []


def test_modes_all_writes_the_files_it_always_wrote(tmp_path):
    d = _make(tmp_path)
    out = tmp_path / "all"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0001.png", "--gpu-only", "--radius", 4, "--outdir", out])      # --modes all is the default
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(f"output-{m}.png" for m in (
        "nonlinear-bialteral", "nonlinear-bialteral-layers", "linear-bialteral", "nonlinear-nlm", "nonlinear-nlm-multiframe",
        "nonlinear-nlm-multiframe-overlap"))
    assert "joint" not in r.stdout
