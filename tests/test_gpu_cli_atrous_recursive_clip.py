"""GPU suite: mi_denoise --animation --animation-filter atrous-recursive --history-clip GAMMA [--history-clip-radius R] on tiny
frames: the 4-frame PNG animation and the 3-frame EXR animation of the other CLI tests, with --albedo-layer and the firefly clamp
(the box is then taken from the clamped illumination) and without.  Every output file holds the bits of
Context.sequence_atrous_recursive(..., clip_gamma=GAMMA, clip_radius=R) on the arrays the files decode to; the run prints its
`history-clip radius <r> gamma <g>` line; two frame blocks whose warm-up reaches frame 0 equal the unsharded run; the options with
another filter, the radius without --history-clip and out-of-range values are refused with nothing written."""
import os

import numpy as np
import pytest

from test_gpu_cli_atrous_recursive_firefly import _check
from test_gpu_cli_atrous_temporal import COUNT, SIGMAS, _bits, _decoded, _make, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_albedo", (False, True), ids=("colour", "albedo-layer"))
@pytest.mark.parametrize("kind", ["png", "exr"])
def test_the_history_clip_options_run_the_python_sequence_bits(tmp_path, ctx, kind, with_albedo):
    d = _make(tmp_path, kind)
    n = COUNT[kind]
    frames, layers = _decoded(d, kind)                       # layers[i] = [albedo, normal]
    if with_albedo:
        albedo, guides, sig = [ls[0] for ls in layers], [[ls[1]] for ls in layers], [SIGMAS[kind][1]]
        extra, ff = ["--albedo-layer", "albedo", "--firefly-rank", 2], dict(firefly_rank=2)
    else:
        albedo, guides, sig, extra, ff = None, layers, SIGMAS[kind], [], {}
    out_dt = np.uint8 if kind == "png" else np.float32
    base = [d / f"Animation01_X_0000.{kind}", "--animation", "--animation-filter", "atrous-recursive", "--gpu-only", "--sigma-layers",
            ",".join(str(s) for s in sig), "--passes", 3] + extra
    kw = dict(passes=3, out_dtype=out_dt, albedo=albedo, **ff)

    runs = (("a", ["--history-clip", 1], dict(clip_gamma=1.0), "history-clip radius 1 gamma 1"),
            ("b", ["--history-clip", "0.5", "--history-clip-radius", 2], dict(clip_gamma=0.5, clip_radius=2), "history-clip radius 2 gamma 0.5"),
            ("z", ["--history-clip", 0], dict(clip_gamma=0.0), "history-clip radius 1 gamma 0"))
    wants = {}
    for sub, more, clip, shown in runs:
        out = tmp_path / sub
        out.mkdir()
        r = _run(tmp_path, base + more + ["--outdir", out])
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln.strip() for ln in r.stdout.splitlines()]
        assert [ln for ln in lines if ln.startswith("history-clip ")] == [shown], r.stdout
        want, _ = ctx.sequence_atrous_recursive(frames, guides, sig, **clip, **kw)
        _check(out, kind, want)
        wants[sub] = want
    plain, _ = ctx.sequence_atrous_recursive(frames, guides, sig, **kw)
    assert np.array_equal(_bits(wants["b"][0]), _bits(plain[0]))                 # frame 0 has no history to clip ...
    assert any(not np.array_equal(_bits(w), _bits(p)) for w, p in zip(wants["b"][1:], plain[1:]))       # ... the later ones do

    # without the option: no line, the existing bits
    out = tmp_path / "p"
    out.mkdir()
    r = _run(tmp_path, base + ["--outdir", out])
    assert r.returncode == 0 and not any(ln.strip().startswith("history-clip ") for ln in r.stdout.splitlines()), r.stdout + r.stderr
    _check(out, kind, plain)

    # two frame blocks through the same stage function, their warm-up calls too: the whole run's bits when the warm-up reaches frame 0
    out = tmp_path / "c"
    out.mkdir()
    r = _run(tmp_path, base + ["--history-clip", "0.5", "--history-clip-radius", 2, "--gpus", 2, "--share-device", "--warmup", n, "--outdir", out])
    assert r.returncode == 0, r.stdout + r.stderr
    _check(out, kind, wants["b"])


def test_refusals_write_nothing(tmp_path):
    d = _make(tmp_path, "png")
    anim = [d / "Animation01_X_0000.png", "--animation", "--gpu-only"]
    rec = anim + ["--animation-filter", "atrous-recursive"]
    only = "applies to --animation --animation-filter atrous-recursive only"
    cases = ((anim + ["--animation-filter", "atrous-variance", "--history-clip", 1], ["--history-clip " + only]),
             (anim + ["--animation-filter", "atrous", "--history-clip-radius", 2], ["--history-clip-radius " + only]),
             (anim + ["--history-clip", "1.5"], ["--history-clip " + only]),
             ([d / "Animation01_X_0000.png", "--gpu-only", "--modes", "atrous-variance", "--history-clip", 2], ["--history-clip " + only]),
             (rec + ["--history-clip-radius", 2], ["--history-clip-radius needs --history-clip"]),
             (rec + ["--history-clip", 1, "--history-clip-radius", 3], ["--history-clip-radius 3 is neither 1 nor 2"]),
             (rec + ["--history-clip", 1, "--history-clip-radius", 0], ["--history-clip-radius 0 is neither 1 nor 2"]),
             (rec + ["--history-clip", "-1"], ["--history-clip -1 must be finite and >= 0"]),
             (rec + ["--history-clip", "inf"], ["--history-clip inf must be finite and >= 0"]),
             (rec + ["--history-clip", "nan"], ["--history-clip nan must be finite and >= 0"]))
    for j, (args, needles) in enumerate(cases):
        out = tmp_path / f"r{j}"
        out.mkdir()
        r = _run(tmp_path, args + ["--outdir", out])
        text = r.stdout + r.stderr
        assert r.returncode != 0 and all(x in text for x in needles), text
        assert os.listdir(out) == []
