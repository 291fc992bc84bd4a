"""GPU suite: mi_denoise --animation --animation-filter atrous-recursive --albedo-layer SUBSTR [--albedo-floor X] on tiny frames: the
4-frame PNG animation with .png render elements and the 3-frame EXR animation with .exr ones of the other CLI tests, whose
`albedo_*` element becomes the albedo plane and leaves the guide layers (`normal_*` stays).  Every output file holds the bits of
Context.sequence_atrous_recursive(..., albedo=...) on the arrays the files decode to; the run prints its `albedo <file> floor <x>`
line and no `layer` line for that file; two frame blocks whose warm-up reaches frame 0 equal the unsharded run; a substring that
matches no file or several, an albedo in another format than the guide layers, and the options with another filter are refused
with nothing written."""
import os

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from test_gpu_cli_atrous_temporal import COUNT, SHAPE, SIGMAS, _bits, _decoded, _make, _run

pytestmark = pytest.mark.gpu
INFIX = "output-animation-nonlinear-atrous-recursive-"


def _check(out, kind, want):
    names = sorted(os.listdir(out))
    assert names == [f"{INFIX}Animation01_X_{i:04d}.{kind}" for i in range(COUNT[kind])], names
    for i, name in enumerate(names):
        got = mid.load_image(out / name, None)
        assert got.dtype == want[i].dtype and np.array_equal(_bits(got), _bits(want[i])), i


@pytest.mark.parametrize("kind", ["png", "exr"])
def test_the_albedo_layer_runs_the_python_sequence_bits(tmp_path, ctx, kind):
    d = _make(tmp_path, kind)
    n = COUNT[kind]
    frames, layers = _decoded(d, kind)                       # layers[i] = [albedo, normal]
    albedo, guides, sig = [ls[0] for ls in layers], [[ls[1]] for ls in layers], [SIGMAS[kind][1]]
    out_dt = np.uint8 if kind == "png" else np.float32
    base = [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-recursive", "--gpu-only", "--sigma-layers", sig[0], "--passes", 3,
            "--albedo-layer", "albedo"]
    kw = dict(passes=3, out_dtype=out_dt)

    for sub, more, floor, shown in (("a", [], 1e-3, "0.001"), ("b", ["--albedo-floor", "0.25"], 0.25, "0.25")):
        out = tmp_path / sub
        out.mkdir()
        r = _run(tmp_path, base + more + ["--outdir", out])
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.strip() for ln in r.stdout.splitlines()]
        alb = [ln for ln in lines if ln.startswith("albedo ")]
        assert len(alb) == 1 and alb[0].endswith(f"albedo_0000.{kind} floor {shown}"), r.stdout
        lay = [ln for ln in lines if ln.startswith("layer ")]
        assert len(lay) == 1 and f"normal_0000.{kind}" in lay[0] and not any("albedo_0000" in ln for ln in lay), r.stdout
        want, _ = ctx.sequence_atrous_recursive(frames, guides, sig, albedo=albedo, albedo_floor=floor, **kw)
        _check(out, kind, want)
    plain, _ = ctx.sequence_atrous_recursive(frames, guides, sig, **kw)
    assert not np.array_equal(_bits(want[-1]), _bits(plain[-1]))                         # the albedo counts

    # two frame blocks: the albedo planes are staged from the host like the layers; the whole run's bits when the warm-up reaches frame 0
    whole, _ = ctx.sequence_atrous_recursive(frames, guides, sig, albedo=albedo, **kw)
    out = tmp_path / "c"
    out.mkdir()
    r = _run(tmp_path, base + ["--gpus", 2, "--share-device", "--warmup", n, "--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    _check(out, kind, whole)


def test_refusals_write_nothing(tmp_path):
    # directory A: a second .png element whose name contains "albedo"; directory B: an .exr element beside the .png guide layers
    d, db = _make(tmp_path / "A", "png"), _make(tmp_path / "B", "png")
    for i in range(COUNT["png"]):
        mid.save_image(d / "RenderElements" / f"albedo2_{i:04d}.png", np.full(SHAPE + (4,), 128, np.uint8))
        mid.save_image(db / "RenderElements" / f"diffuse_{i:04d}.exr", np.full(SHAPE + (4,), 0.5, np.float32))
    anim = [d / "Animation01_X_0000.png", "--animation", "--gpu-only"]
    rec = anim + ["--animation-filter", "atrous-recursive"]
    mixed = [db / "Animation01_X_0000.png", "--animation", "--gpu-only", "--animation-filter", "atrous-recursive"]
    cases = ((rec + ["--albedo-layer", "nothing"], ["--albedo-layer nothing matches 0 layer file(s)"]),
             (rec + ["--albedo-layer", "albedo"], ["--albedo-layer albedo matches 2 layer file(s)"]),
             (mixed + ["--albedo-layer", "diffuse"], ["diffuse_0000.exr is an .exr", "all guide layers of a run must have one format"]),
             (rec + ["--albedo-layer", "albedo2", "--albedo-floor", "0"], ["floor 0 must be finite and > 0"]),
             (rec + ["--albedo-floor", "0.1"], ["--albedo-floor needs --albedo-layer"]),
             (anim + ["--animation-filter", "atrous-variance", "--albedo-layer", "albedo2"], ["--albedo-layer applies to --animation --animation-filter atrous-recursive only"]),
             (anim + ["--animation-filter", "atrous", "--albedo-floor", "0.1"], ["--albedo-floor applies to --animation --animation-filter atrous-recursive only"]),
             ([d / "Animation01_X_0000.png", "--gpu-only", "--modes", "atrous", "--albedo-layer", "albedo2"], ["--albedo-layer applies to"]))
    for j, (args, needles) in enumerate(cases):
        out = tmp_path / f"r{j}"
        out.mkdir()
        r = _run(tmp_path, args + ["--outdir", out])
        text = r.stdout + r.stderr
        assert r.returncode != 0 and all(x in text for x in needles), text
        assert os.listdir(out) == []
