"""GPU suite: what the metrics are for.  A synthetic noisy 8-frame 131 x 67 sequence whose clean frames are known (a static scene of
three smoothly shaded surfaces, path-tracer-like multiplicative noise, a label layer as the guide): the output of
sequence_atrous_recursive at the last frame is closer to the clean frame than the noisy input is -- lower mse, lower relmse, higher
ssim, by mid_image_metrics.  Only the ordering is asserted (no margin is fixed in advance), after the checker has confirmed on the CPU
that the input is far from perfect (ssim < 0.8) and that the GPU's metrics of the input are the checker's."""
import numpy as np
import pytest

import np_image_metrics as M

pytestmark = pytest.mark.gpu
H, W, N = 67, 131, 8


def scene():
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    label = np.where(xx + 0.5 * yy < 60, 40, np.where(yy > 40, 200, 120)).astype(np.uint8)
    shade = 0.35 + 0.3 * np.sin(xx * 0.03 + 0.5) * np.cos(yy * 0.04)
    tint = {40: (0.9, 0.5, 0.3), 120: (0.3, 0.7, 0.9), 200: (0.6, 0.9, 0.4)}
    clean = np.ones((H, W, 4))
    for v, t in tint.items():
        clean[label == v, :3] = shade[label == v][:, None] * np.array(t) * (0.6 + v / 250.0)
    layer = np.repeat(label[..., None], 4, -1)
    layer[..., 3] = 255
    return clean.astype(np.float32), layer


def test_the_filter_brings_the_sequence_closer_to_the_clean_frame(ctx):
    clean, layer = scene()
    rng = np.random.default_rng(11)
    noisy = []
    for _ in range(N):
        f = clean.copy()
        f[..., :3] *= rng.gamma(4.0, 0.25, (H, W, 1)).astype(np.float32)            # mean 1, standard deviation 0.5
        noisy.append(f)
    ref_in = M.image_metrics(noisy[-1], clean)
    assert ref_in["ssim"] < 0.8 and ref_in["mse"] > 1e-3                            # by the checker: the input is far from perfect
    out, _ = ctx.sequence_atrous_recursive(noisy, [[layer]] * N, [0.1], warmup=N, passes=4)
    assert len(out) == N and np.isfinite(out[-1]).all()
    before, after = ctx.image_metrics(noisy[-1], clean), ctx.image_metrics(out[-1], clean)
    assert before["ssim"] == pytest.approx(ref_in["ssim"], abs=1e-9) and before["mse"] == pytest.approx(ref_in["mse"], rel=1e-12)
    for k in ("mse", "relmse", "ssim", "psnr", "mae"):
        print(f"{k}: noisy input {before[k]!r}, filtered output {after[k]!r}")
    assert after["mse"] < before["mse"]
    assert after["relmse"] < before["relmse"]
    assert after["ssim"] > before["ssim"]
