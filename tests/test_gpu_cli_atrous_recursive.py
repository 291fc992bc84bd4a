"""GPU suite: mi_denoise --animation --animation-filter atrous-recursive -- --alpha, --alpha-moments, --history-max, --feedback,
--warmup, --motion-layer, --motion-scale, --passes, --sigma-layers, frame blocks over --gpus -- on tiny frames: a 4-frame PNG
animation with .png layers and a 3-frame EXR animation with .exr layers, each with an .exr motion element the test writes
through save_image.  Every output file holds the bits of Context.sequence_atrous_recursive on the arrays the files decode to; the
run prints its `motion <file> scale <sx> <sy>` line; a .png motion layer, a substring that matches no file or several, --halo
rccl and --modes atrous-recursive are refused with nothing written; the help text says when a sharded run equals the whole one."""
import os

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from test_gpu_cli_atrous_temporal import COUNT, LAYERS, SHAPE, SIGMAS, _bits, _decoded, _make, _run

pytestmark = pytest.mark.gpu
INFIX = "output-animation-nonlinear-atrous-recursive-"


def _motion(i):
    h, w = SHAPE
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    m = np.zeros((h, w, 4), np.float32)
    m[..., 0] = 2.5 * np.sin(xx * 0.2 + i) + 0.25
    m[..., 1] = 1.5 * np.cos(yy * 0.3 + xx * 0.1) - 0.5 * i
    m[..., 2] = 9.0                                    # (B and A are not motion)
    return m


def _with_motion(d, kind, name="velocity"):
    for i in range(COUNT[kind]):
        mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.exr", _motion(i))
    return [mid.load_image(d / "RenderElements" / f"{name}_{i:04d}.exr", None) for i in range(COUNT[kind])]


def _check(out, kind, want):
    names = sorted(os.listdir(out))
    assert names == [f"{INFIX}Animation01_X_{i:04d}.{kind}" for i in range(COUNT[kind])], names
    for i, name in enumerate(names):
        got = mid.load_image(out / name, None)
        assert got.dtype == want[i].dtype and np.array_equal(_bits(got), _bits(want[i])), i


@pytest.mark.parametrize("kind", ["png", "exr"])
def test_atrous_recursive_writes_the_python_sequence_bits(tmp_path, ctx, kind):
    d = _make(tmp_path, kind)
    n = COUNT[kind]
    frames, layers = _decoded(d, kind)
    sig = SIGMAS[kind]
    out_dt = np.uint8 if kind == "png" else np.float32
    base = [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-recursive", "--gpu-only", "--sigma-layers", ",".join(str(s) for s in sig)]

    # 1. no motion layer: zero motion, the defaults (feedback 1, warm-up 16, alpha 0.2, five passes)
    out = tmp_path / "a"
    out.mkdir()
    r = _run(tmp_path, base + ["--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "motion " not in r.stdout
    still, _ = ctx.sequence_atrous_recursive(frames, layers, sig, out_dtype=out_dt)
    _check(out, kind, still)

    # 2. the motion element: taken out of the guide layers, scaled, announced
    mv = _with_motion(d, kind)
    planes = [m[..., :2] * np.float32([0.5, -2.0]) for m in mv]
    opts = ["--motion-layer", "veloc", "--motion-scale", "0.5,-2", "--alpha", 0.1, "--alpha-moments", 0.3, "--history-max", 3, "--passes", 3]
    kw = dict(alpha=0.1, alpha_moments=0.3, history_max=3, passes=3, out_dtype=out_dt)
    for sub, more, seq in (("b", ["--feedback", 0], dict(feedback=0)), ("c", ["--feedback", 1], dict(feedback=1))):
        out = tmp_path / sub
        out.mkdir()
        r = _run(tmp_path, base + opts + more + ["--outdir", out])
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.strip() for ln in r.stdout.splitlines() if ln.strip().startswith("motion ")]
        assert len(lines) == 1 and lines[0].endswith("velocity_0000.exr scale 0.5 -2"), r.stdout
        assert not any("velocity" in ln for ln in r.stdout.splitlines() if ln.strip().startswith("layer ")), r.stdout
        want, _ = ctx.sequence_atrous_recursive(frames, layers, sig, motion=planes, **seq, **kw)
        _check(out, kind, want)
        assert not np.array_equal(_bits(want[-1]), _bits(ctx.sequence_atrous_recursive(frames, layers, sig, **seq, **kw)[0][-1]))   # the motion counts

    # 3. two frame blocks: each starts its history --warmup frames before its block; the whole run's bits only when that reaches frame 0
    whole, _ = ctx.sequence_atrous_recursive(frames, layers, sig, motion=planes, feedback=1, **kw)
    for sub, warm in (("d", 0), ("e", n)):
        out = tmp_path / sub
        out.mkdir()
        r = _run(tmp_path, base + opts + ["--gpus", 2, "--share-device", "--warmup", warm, "--outdir", out])
        assert r.returncode == 0, r.stdout + r.stderr
        want = []
        for g in range(2):
            start, count = mid.shard_block(n, 2, g)
            want += ctx.sequence_atrous_recursive(frames, layers, sig, motion=planes, feedback=1, warmup=warm, first=start, count=count, **kw)[0]
        _check(out, kind, want)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(want, whole)) == (warm == n)


def test_refusals_write_nothing_and_help_states_the_warm_up_rule(tmp_path):
    # directory A: two .exr elements whose names contain "velocity", and a .png one; directory B: one motion element
    da, d = _make(tmp_path / "A", "png"), _make(tmp_path / "B", "png")
    _with_motion(da, "png")
    _with_motion(da, "png", "velocity2")
    _with_motion(d, "png")
    for i in range(COUNT["png"]):
        mid.save_image(da / "RenderElements" / f"flow_{i:04d}.png", np.zeros(SHAPE + (4,), np.uint8))
    tail = ["--animation", "--animation-filter", "atrous-recursive", "--gpu-only"]
    bad, anim = [da / "Animation01_X_0000.png"] + tail, [d / "Animation01_X_0000.png"] + tail
    cases = ((bad + ["--motion-layer", "flow"], ["motion layer", "is a .png"]),
             (bad + ["--motion-layer", "nothing"], ["--motion-layer nothing matches 0 layer file(s)"]),
             (bad + ["--motion-layer", "velocity"], ["--motion-layer velocity matches 2 layer file(s)"]),
             (anim + ["--motion-layer", "velocity", "--halo", "rccl"], ["--halo rccl is not available with --animation-filter atrous-recursive"]),
             (anim + ["--motion-layer", "velocity", "--alpha", "0"], ["alpha"]),
             (anim + ["--motion-layer", "velocity", "--history-max", "0.5"], ["historyMax"]),
             (anim + ["--feedback", "2"], ["--feedback 2 is neither 0 nor 1"]),
             (anim + ["--warmup", "-1"], ["--warmup -1 is negative"]))
    for j, (args, needles) in enumerate(cases):
        out = tmp_path / f"r{j}"
        out.mkdir()
        r = _run(tmp_path, args + ["--outdir", out])
        text = r.stdout + r.stderr
        assert r.returncode != 0 and all(x in text for x in needles), text
        assert os.listdir(out) == []
    out = tmp_path / "m"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0000.png", "--modes", "atrous-recursive", "--gpu-only", "--outdir", out])
    assert r.returncode != 0 and "--animation-filter atrous-recursive" in r.stdout + r.stderr and os.listdir(out) == []
    r = _run(tmp_path, [d / "Animation01_X_0000.png", "--animation", "--animation-filter", "atrous", "--motion-layer", "velocity", "--gpu-only", "--outdir", out])
    assert r.returncode != 0 and "--motion-layer applies to --animation-filter atrous-recursive only" in r.stdout + r.stderr and os.listdir(out) == []
    h = _run(tmp_path, ["--help"]).stdout
    assert "or atrous-recursive:" in h and "output-animation-nonlinear-atrous-recursive-*" in h
    assert "equals the unsharded one bit for bit only when the warm-up reaches frame 0" in " ".join(h.split())
    for o in ("--alpha X", "--alpha-moments X", "--history-max N", "--feedback 0|1", "--warmup N", "--motion-layer SUBSTR", "--motion-scale SX,SY"):
        assert o in h, o
