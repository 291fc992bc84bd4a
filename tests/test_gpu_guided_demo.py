"""GPU suite: what the guided filter is for.  A 70 x 130 frame of noisy `albedo x smooth light` (gamma noise of standard deviation
0.5) with the clean, blocky albedo as the guide: by Context.image_metrics the guided output at radius 8 is closer to the clean frame
than the input and than Context.bilateral_joint guided by the same layer at radius 8 -- and the same call guided by the frame itself
is not: the guide is the point.  The two MSE ratios asserted are the float64 checker's (tests/test_guided_args.py asserts them of the
contract on the CPU); the margin is what the header's precision clause lets the kernel's MSE differ from the checker's by."""
import numpy as np
import pytest

import guided_inputs as gi
import np_guided

pytestmark = pytest.mark.gpu


def test_the_guide_is_the_point(ctx):
    noisy, alb, clean = gi.demo()
    r, eps = gi.DEMO_RADIUS, gi.DEMO_EPS
    guided, selfg = ctx.guided_filter(noisy, alb, r, eps), ctx.guided_filter(noisy, None, r, eps)
    joint = ctx.bilateral_joint([noisy], [[alb]], radius=r)[0]
    m = {name: ctx.image_metrics(x, clean, ssim=False)["mse"] for name, x in (("input", noisy), ("guided", guided), ("self-guided", selfg),
                                                                            ("joint bilateral", joint))}
    print(", ".join(f"mse {k} {v:.5f}" for k, v in m.items()))
    # the kernel's MSE against the checker's: |out - exact| <= e = 8 * 2^-24 * max T moves an MSE by at most 2 sqrt(mse) e + e^2
    for got, guide in ((m["guided"], alb), (m["self-guided"], None)):
        ref = np_guided.guided(noisy, guide, r, eps)
        want = float(((ref["out"][..., :3] - clean[..., :3].astype(np.float64)) ** 2).mean())
        e = float(np_guided.tolerance(ref).max())
        assert abs(got - want) <= 2 * np.sqrt(want) * e + e * e + 1e-12 * want
    assert m["guided"] <= gi.DEMO_GUIDED_RATIO * m["input"]
    assert m["self-guided"] >= gi.DEMO_SELF_RATIO * m["guided"]
    assert m["guided"] < m["joint bilateral"]
