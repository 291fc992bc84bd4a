"""GPU suite: mi_denoise --compare TEST REFERENCE [--peak X] [--relmse-eps X] [--no-ssim] [--half] [--animation] on tiny files.
.png against .png, .exr against .png and --half: the printed numbers parse back to Context.image_metrics's on the arrays the files
decode to, bit for bit; an --animation run over four pairs with its mean line; --no-ssim; every refusal, on stderr with nothing on
stdout; no file is written."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import image_denoising_filter_amd as mid
from image_metrics_inputs import as_dtype, pair

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
KEYS = {"n": "n_valid", "invalid": "n_invalid", "mse": "mse", "psnr": "psnr", "mae": "mae", "max": "max_abs", "relmse": "relmse", "ssim": "ssim"}
H, W = 21, 70


def run(args, cwd):
    return subprocess.run([CLI] + [str(x) for x in args], cwd=cwd, capture_output=True, text=True, timeout=300)


def parse(line):
    """`metrics <test> vs <reference> n <..> invalid <..> ...` or `metrics mean over <n> frames n <..> ...` -> (head words, values by result name)."""
    words = line.split()
    at = words.index("n", 4)
    body = words[at:]
    assert body[0::2] == list(KEYS), line
    return words[:at], {KEYS[k]: float(v) for k, v in zip(body[0::2], body[1::2])}


def same(x, y):
    return x == y or (math.isnan(x) and math.isnan(y))


def write_pair(d, i, seed=0):
    """frame i of a test sequence (noisy) and of its reference, as .png and as .exr; an .exr test frame carries a NaN texel."""
    a, b = pair(H, W, seed=seed + i)
    for sub in ("test", "ref"):
        os.makedirs(d / sub, exist_ok=True)
    ea = a.copy()
    ea[3 + i, 5, 1] = np.nan
    mid.save_image(d / "test" / f"out_{i:04d}.png", as_dtype(a, np.uint8))
    mid.save_image(d / "test" / f"out_{i:04d}.exr", ea)
    mid.save_image(d / "ref" / f"Render_{i:04d}.png", as_dtype(b, np.uint8))
    mid.save_image(d / "ref" / f"Render_{i:04d}.exr", b)


def test_single_pairs_print_the_python_methods_bits(tmp_path, ctx):
    write_pair(tmp_path, 0)
    before = sorted(os.listdir(tmp_path))
    t, r = tmp_path / "test" / "out_0000", tmp_path / "ref" / "Render_0000"
    cases = (([f"{t}.png", f"{r}.png"], {}, (None, None)),
             ([f"{t}.exr", f"{r}.png"], {}, (None, None)),
             ([f"{t}.exr", f"{r}.exr", "--half"], {}, (np.float16, np.float16)),
             ([f"{t}.png", f"{r}.exr", "--half", "--peak", "0.5", "--relmse-eps", "0.001"], dict(peak=0.5, eps=0.001), (None, np.float16)),
             ([f"{t}.exr", f"{r}.exr", "--no-ssim"], dict(ssim=False), (None, None)),
             ([f"{r}.exr", f"{r}.exr"], {}, (None, None)))
    for args, kw, dts in cases:
        res = run(["--compare"] + args, tmp_path)
        assert res.returncode == 0, res.stdout + res.stderr
        lines = res.stdout.splitlines()
        assert len(lines) == 1 and lines[0].startswith(f"metrics {args[0]} vs {args[1]} n "), res.stdout
        _, got = parse(lines[0])
        a = mid.load_image(args[0], dtype=dts[0] if args[0].endswith(".exr") else None)
        b = mid.load_image(args[1], dtype=dts[1] if args[1].endswith(".exr") else None)
        want = ctx.image_metrics(a, b, **kw)
        for k in got:
            assert same(got[k], want[k]), (args, k, got[k], want[k])
        assert got["n_invalid"] == (1 if args[0].endswith("0000.exr") and "out_" in args[0] else 0)
        assert math.isnan(got["ssim"]) == ("--no-ssim" in args)
    _, got = parse(run(["--compare", f"{r}.exr", f"{r}.exr"], tmp_path).stdout.splitlines()[0])
    assert got["mse"] == 0 and got["psnr"] == math.inf and got["ssim"] == 1.0
    assert sorted(os.listdir(tmp_path)) == before and len(os.listdir(tmp_path / "test")) == 2          # nothing was written


def test_an_animation_of_four_pairs_and_its_mean(tmp_path, ctx):
    for i in range(4):
        write_pair(tmp_path, i, seed=40)
    res = run(["--compare", tmp_path / "test" / "out_0002.png", tmp_path / "ref" / "Render_0000.exr", "--animation"], tmp_path)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 5
    per = []
    for i, line in enumerate(lines[:4]):
        ta, rb = tmp_path / "test" / f"out_{i:04d}.png", tmp_path / "ref" / f"Render_{i:04d}.exr"
        head, got = parse(line)
        assert head == ["metrics", str(ta), "vs", str(rb)]
        want = ctx.image_metrics(mid.load_image(ta), mid.load_image(rb))
        assert all(same(got[k], want[k]) for k in got), line
        per.append(got)
    head, mean = parse(lines[4])
    assert head == ["metrics", "mean", "over", "4", "frames"]
    for k in mean:
        m = 0.0
        for g in per:
            m += g[k]
        assert mean[k] == m / 4.0, k
    assert len({g["mse"] for g in per}) == 4


def test_refusals(tmp_path):
    for i in range(2):
        write_pair(tmp_path, i)
    t, r = tmp_path / "test", tmp_path / "ref"
    a, _ = pair(H + 1, W)
    mid.save_image(tmp_path / "taller.png", as_dtype(a, np.uint8))
    os.makedirs(tmp_path / "lonely")
    os.makedirs(tmp_path / "twice")
    os.makedirs(tmp_path / "shared")
    for name, dst in (("out_0000.png", "lonely/out_0000.png"), ("out_0001.png", "lonely/out_0007.png"), ("out_0000.png", "shared/x_0001.png"),
                      ("out_0001.png", "shared/y_0001.png")):
        os.link(t / name, tmp_path / dst)
    for name, dst in (("Render_0000.png", "twice/A_0000.png"), ("Render_0001.png", "twice/B_0000.png"), ("Render_0001.png", "twice/B_0001.png")):
        os.link(r / name, tmp_path / dst)
    cases = (([tmp_path / "taller.png", r / "Render_0000.png"], [f"{W}x{H + 1}", f"{W}x{H}", "taller.png", "Render_0000.png"]),
             ([t / "out_0000.png", r / "missing.png"], ["missing.png"]),
             ([t / "out_0000.exr", r / "Render_0000.png", "--peak", "0"], ["--peak 0 must be finite and > 0"]),
             ([t / "out_0000.exr", r / "Render_0000.png", "--relmse-eps", "nan"], ["--relmse-eps nan must be finite and > 0"]),
             ([t / "out_0000.png", r / "Render_0000.png", "--modes", "nlm"], ["--modes"]),
             ([t / "out_0000.png", r / "Render_0000.png", "--gpus", 2], ["--gpus"]),
             ([t / "out_0000.png", r / "Render_0000.png", "--animation", "--animation-filter", "atrous"], ["--animation-filter"]),
             ([tmp_path / "lonely" / "out_0000.png", r / "Render_0000.png", "--animation"], ["out_0007.png", "no partner"]),
             ([t / "out_0000.png", tmp_path / "twice" / "A_0000.png", "--animation"], ["out_0000.png", "two partners", "A_0000.png", "B_0000.png"]),
             ([tmp_path / "shared" / "x_0001.png", r / "Render_0000.png", "--animation"], ["x_0001.png", "y_0001.png", "share"]))
    for args, needles in cases:
        res = run(["--compare"] + list(args), tmp_path)
        assert res.returncode != 0 and all(x in res.stderr for x in needles), (args, res.stdout, res.stderr)
        assert res.stdout == ""                                     # stdout holds `metrics` lines only: every refusal goes to stderr
