"""GPU suite: what a plain `bench.py` run does and what `--dump-outputs` writes.

A plain run is the headline alone (set up, warm up, K timed steps, the line); everything else waits for --full.
--dump-outputs DIR holds what the timed path computed in its last step: frame 0 in full and a seeded sample of every frame,
float32, within 64 MiB, and it must be what a caller of the same path gets for the same (seeded) frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu


def test_plain_run_is_the_headline_and_dumps_the_last_steps_outputs(tmp_path, ctx):
    import bench
    import image_denoising_filter_amd as mid
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:2000]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mpixel/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("Mpixel/s (NLM")
    # the value is the steps' pixels over the steps' time
    assert abs(d["value"] - 2 * bench.NPIX / 1e3 / d["ms_per_step"]) / d["value"] < 0.01
    # nothing beyond the headline without --full
    assert d["also"] == {} and d["cpu_baseline"] is None and "single_frame_launch" not in d["config"] and "scaling_strong" not in d

    files = sorted(os.listdir(out))
    assert files == ["outputs_frame0.npy", "outputs_sample.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    f0, s = np.load(out / "outputs_frame0.npy"), np.load(out / "outputs_sample.npy")
    n = bench.DUMP_SAMPLE_PX // 2
    assert f0.dtype == np.float32 and f0.shape == (bench.H, bench.W, 4)
    assert s.dtype == np.float32 and s.shape == (2, n, 4)

    # the same seeded frames (rank 0's seed) through the library's own temporal NLM call, k = 0
    frames = [f.cpu().numpy() for f in bench.synth_frames(2, 100, torch.device("cuda", 0))]
    want = ctx.nlm_temporal(frames, k=0, hparam=bench.HPARAM, **mid.NLM_BENCH)
    assert rel_err(f0, want[0]) < 1e-5
    idx = np.sort(np.random.default_rng(0).choice(bench.NPIX, size=n, replace=False))
    for i in range(2):
        assert rel_err(s[i], want[i].reshape(-1, 4)[idx]) < 1e-5
