"""CPU: the float64 checker of the variance-guided a-trous filter (np_atrous_variance.py) against answers known without it."""
import numpy as np

import np_atrous_joint as joint
import np_atrous_variance as chk


def _noise_frame(shape, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.gamma(4.0, 0.25, shape + (3,)), np.ones(shape + (1,))], -1).astype(np.float32)


def _layers(shape, L, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.random(shape + (4,)).astype(np.float32) for _ in range(L)]


def test_a_constant_frame_has_no_variance_and_stays_constant():
    shape = (19, 23)
    fr = np.broadcast_to(np.array([0.3, 2.5, 0.01, 0.7], np.float32), shape + (4,)).copy()
    ly = [_layers(shape, 2, seed=f) for f in range(3)]
    for k in (0, 1):
        v0, m2 = chk.moments([fr] * 3, ly, [0.4, 0.6], k=k, t=1)
        assert np.array_equal(v0, np.zeros(shape)) and np.array_equal(m2, np.zeros(shape))
    C, V = chk.atrous_variance(fr, np.zeros(shape, np.float32), ly[1], [0.4, 0.6], passes=5, sigma_lum=4.0, epsilon=1e-3)
    assert np.abs(C - fr).max() <= 1e-14 and np.array_equal(V, np.zeros(shape))


def test_without_the_luminance_term_the_colour_is_the_joint_filter():
    shape = (21, 30)
    fr, ly, sg = _noise_frame(shape), _layers(shape, 3), [0.3, 0.5, 0.4]
    v = np.random.default_rng(1).random(shape).astype(np.float32)
    for passes, first in ((1, 0), (3, 0), (2, 2)):
        C, _ = chk.atrous_variance(fr, v, ly, sg, passes=passes, first_pass=first, sigma_lum=0.0)
        ref = joint.atrous_joint(fr, ly, sg, passes=passes, first_pass=first, color_sigma=0.0)
        assert np.abs(C - ref).max() <= 1e-13


def test_constant_guides_propagate_a_constant_variance_by_the_kernel_norm():
    """All weights are K(o): V_1 = V sum K^2 / (sum K)^2 = V (70 / 256)^2 where all 25 taps lie inside the image."""
    shape = (20, 24)
    fr = _noise_frame(shape)
    ly = [np.full(shape + (4,), 0.25, np.float32)]
    for step, first in ((1, 0), (4, 2)):
        _, V = chk.atrous_variance(fr, np.full(shape, 3.0, np.float32), ly, [0.5], passes=1, first_pass=first, sigma_lum=0.0)
        m = 2 * step
        assert np.abs(V[m:-m, m:-m] - 3.0 * (70.0 / 256.0) ** 2).max() <= 1e-15
        assert V[0, 0] > 3.0 * (70.0 / 256.0) ** 2                  # fewer taps at the corner: less averaging


def test_moments_of_a_step_frame_with_guides_that_separate_the_levels():
    h, w = 16, 30
    fr = np.empty((h, w, 4), np.float32)
    fr[:, :w // 2] = (0.25, 0.5, 1, 1)
    fr[:, w // 2:] = (3, 2, 0.125, 0.5)
    g = np.zeros((h, w, 4), np.float32)
    g[:, w // 2:, :3] = 1.0
    v0, m2 = chk.moments([fr], [[g]], [0.02], k=0, t=0)
    assert np.array_equal(v0, np.zeros((h, w))) and np.abs(m2).max() < 1e-300
    # without the guide's edge the pixels next to the step see both levels
    v1, _ = chk.moments([fr], [[np.zeros_like(g)]], [0.02], k=0, t=0)
    assert v1[:, w // 2 - 3:w // 2 + 3].min() > 0.1 and np.array_equal(v1[:, :w // 2 - 3], np.zeros((h, w // 2 - 3)))


def test_taps_outside_the_image_are_skipped_at_a_corner():
    shape = (9, 11)
    fr = _noise_frame(shape)
    flat = [np.zeros(shape + (4,), np.float32)]                     # every weight is 1
    v0, m2 = chk.moments([fr], [flat], [1.0], k=0, t=0)
    lum = chk.lum(fr.astype(np.float64))
    assert abs(v0[0, 0] - lum[:4, :4].var()) <= 1e-14               # the 4 x 4 in-image taps of the corner, not 49 with zeros
    assert abs(v0[-1, -1] - lum[-4:, -4:].var()) <= 1e-14
    assert abs(v0[4, 5] - lum[1:8, 2:9].var()) <= 1e-14
    v = np.random.default_rng(2).random(shape)
    vt = chk.smooth_variance(v)
    assert abs(vt[0, 0] - (4 * v[0, 0] + 2 * v[0, 1] + 2 * v[1, 0] + v[1, 1]) / 9) <= 1e-15
    assert abs(vt[0, 3] - (4 * v[0, 3] + 2 * v[0, 2] + 2 * v[0, 4] + 2 * v[1, 3] + v[1, 2] + v[1, 4]) / 12) <= 1e-15
    # a pass on a 1 x 1 frame has the centre tap alone
    C, V = chk.atrous_variance(fr[:1, :1], np.array([[2.0]]), [flat[0][:1, :1]], [1.0], passes=3, sigma_lum=4.0)
    assert np.array_equal(C, fr[:1, :1].astype(np.float64)) and V[0, 0] == 2.0
