"""GPU suite: what the median is for.  On the recipe's impulse-plus-gamma-noise frame (5 % of the pixels replaced by 0 or 50) at radius
2, three claims, with the constants tests/test_median_args.py measured in float64 and tests/median_inputs.py records with a factor-2
margin: the plain median is closer to the clean frame than the input; the layer-weighted median is closer still; the joint bilateral
at the same radius and layers is not -- a weighted mean cannot leave an outlier out."""
import pytest

import median_inputs as mi

pytestmark = pytest.mark.gpu


def test_the_median_removes_impulses_and_the_layers_keep_the_edges(ctx):
    noisy, g0, clean = mi.demo()
    r, sigmas = mi.DEMO_RADIUS, [mi.DEMO_SIGMA]
    plain = ctx.median_filter(noisy, radius=r)
    weighted = ctx.median_filter(noisy, [g0], sigmas, r)
    bilateral = ctx.bilateral_joint([noisy], [[g0]], sigmas, radius=r, sigma_s=2.0)[0]
    m_in, m_plain, m_w, m_b = (mi.mse(x, clean) for x in (noisy, plain, weighted, bilateral))
    print(f"mse against the clean frame: input {m_in:.4g}, plain median {m_plain:.4g}, weighted median {m_w:.4g}, joint bilateral {m_b:.4g}")
    assert m_plain <= mi.DEMO_PLAIN_RATIO * m_in
    assert m_w <= mi.DEMO_WEIGHTED_RATIO * m_plain
    assert m_b >= mi.DEMO_BILATERAL_RATIO * m_w
