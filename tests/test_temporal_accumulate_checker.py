"""CPU suite: the float64 checker of the recursive temporal accumulation (tests/np_temporal_accumulate.py, section a4j) against
answers worked out by hand: no history, a constant history of length 1, 3 and 7, half-pixel motion, and a fully rejected history."""
import numpy as np
import pytest

from np_temporal_accumulate import tap_geometry, temporal_accumulate

H, W = 5, 7
LR, LG, LB = (float(np.float32(c)) for c in (0.2126, 0.7152, 0.0722))


def grey(v, shape=(H, W)):
    return np.broadcast_to(np.float32([v, v, v, 1.0]), shape + (4,)).copy()


def label(ids):
    return np.stack([ids * 85, ids * 0, ids * 0, ids * 0 + 255], -1).astype(np.uint8)


def test_no_history_is_the_frame_itself():
    fr = np.random.default_rng(0).uniform(0, 2, (H, W, 4)).astype(np.float32)
    vs = np.random.default_rng(1).uniform(0, 1, (H, W)).astype(np.float32)
    r = temporal_accumulate(fr, [], [], [], var_spatial=vs)
    f64 = fr.astype(np.float64)
    l = LR * f64[..., 0] + LG * f64[..., 1] + LB * f64[..., 2]
    assert np.array_equal(r["colour"], fr.astype(np.float64))
    assert np.array_equal(r["state"], np.stack([l, l * l, np.ones((H, W)), np.zeros((H, W))], -1))
    assert np.array_equal(r["variance"], vs.astype(np.float64)) and not r["S"].any()
    assert not temporal_accumulate(fr, [], [], [])["variance"].any()          # Vt = l^2 - l l
    u8 = np.random.default_rng(2).integers(0, 256, (H, W, 4), dtype=np.uint8)
    assert np.array_equal(temporal_accumulate(u8, [], [], [])["colour"], u8 / 255.0)


@pytest.mark.parametrize("n", [1, 3, 7])
def test_a_constant_history_of_length_n(n):
    # frame 0.5 grey, history 0.25 grey with moments (0.25, 0.125) and length n, alpha below 1/8: the blend factor is 1 / (n + 1)
    fr, hc = grey(0.5), grey(0.25)
    st = np.broadcast_to(np.float32([0.25, 0.125, n, 0]), (H, W, 4)).copy()
    ids = np.arange(H * W).reshape(H, W) % 3
    r = temporal_accumulate(fr, [label(ids)], [label(ids)], [0.01], hist=(hc, st), alpha=0.05, alpha_moments=0.05, history_max=32)
    a = 1.0 / (n + 1)
    lsum = LR + LG + LB                                   # l(grey v) = v (LR + LG + LB)
    l = 0.5 * lsum
    assert np.array_equal(r["S"], np.ones((H, W)))
    np.testing.assert_allclose(r["colour"][..., :3], 0.25 + a * 0.25, rtol=0, atol=1e-15)
    assert np.array_equal(r["colour"][..., 3], np.ones((H, W)))
    m1, m2 = 0.25 + a * (l - 0.25), 0.125 + a * (l * l - 0.125)
    np.testing.assert_allclose(r["state"], np.broadcast_to([m1, m2, n + 1.0, 0.0], (H, W, 4)), rtol=0, atol=1e-15)
    np.testing.assert_allclose(r["variance"], m2 - m1 * m1, rtol=0, atol=1e-15)
    # the cap and the floors: historyMax 2 holds N' at 2, alpha 0.75 wins over 1 / N'
    r = temporal_accumulate(fr, [], [], [], hist=(hc, st), alpha=0.75, alpha_moments=1.0, history_max=2)
    np.testing.assert_allclose(r["colour"][..., :3], 0.25 + 0.75 * 0.25, rtol=0, atol=1e-15)
    np.testing.assert_allclose(r["state"], np.broadcast_to([l, l * l, 2.0, 0.0], (H, W, 4)), rtol=0, atol=1e-15)
    # the spatial variance while the history is short: tt = (N' - 1) / (historyFull - 1), 1 from historyFull on
    vs = np.full((H, W), 0.5, np.float32)
    r = temporal_accumulate(fr, [], [], [], hist=(hc, st), var_spatial=vs, alpha=0.05, alpha_moments=0.05, history_full=9)
    vt = m2 - m1 * m1
    np.testing.assert_allclose(r["variance"], 0.5 + min(1.0, n / 8.0) * (vt - 0.5), rtol=0, atol=1e-15)


def test_half_pixel_motion():
    # the history colour is the ramp x, its length 4; every pixel was half a texel further right
    fr = grey(0.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    hc = np.stack([xx, xx, xx, np.ones_like(xx)], -1)
    st = np.broadcast_to(np.float32([0, 0, 4, 0]), (H, W, 4)).copy()
    mv = np.zeros((H, W, 2), np.float32)
    mv[..., 0] = 0.5
    ok, x0, y0, fx, fy = tap_geometry(H, W, mv)
    assert ok.all() and np.array_equal(x0, xx.astype(np.int64)) and np.all(fx == 0.5) and not fy.any()
    r = temporal_accumulate(fr, [], [], [], hist=(hc, st), motion=mv, alpha=1.0, alpha_moments=1.0)    # alpha 1: colour = frame ...
    assert not r["colour"][..., :3].any()
    S = np.ones((H, W))
    S[:, -1] = 0.5                                        # the right tap of the last column lies outside: skipped
    assert np.array_equal(r["S"], S)
    assert np.array_equal(r["state"][..., 2], 4 * S + 1)  # ... and N' counts the unnormalised sum
    r = temporal_accumulate(fr, [], [], [], hist=(hc, st), motion=mv, alpha=0.05, alpha_moments=0.05)
    want = xx.astype(np.float64) + 0.5
    want[:, -1] = W - 1                                   # the one tap left, normalised
    a = 1.0 / (4 * S + 1)
    np.testing.assert_allclose(r["colour"][..., 0], want * (1 - a), rtol=0, atol=1e-14)
    # motion off the frame, NaN and Inf: no history
    for bad in (-(W + 1.0), 1e30, np.nan, np.inf, -np.inf):
        mv[..., 0] = bad
        r = temporal_accumulate(fr, [], [], [], hist=(hc, st), motion=mv, alpha=0.05)
        assert not r["S"].any() and np.array_equal(r["state"][..., 2], np.ones((H, W))) and not r["colour"][..., :3].any()
    mv[..., 0] = -1 + 2.0 ** -24                          # the last position inside: only the right tap, weight 2^-24
    r = temporal_accumulate(fr, [], [], [], hist=(hc, st), motion=mv)
    assert np.all(r["S"][:, 0] == 2.0 ** -24)


def test_a_fully_rejected_history():
    fr = np.random.default_rng(3).uniform(0, 2, (H, W, 4)).astype(np.float32)
    hc = np.random.default_rng(4).uniform(0, 2, (H, W, 4)).astype(np.float32)
    st = np.broadcast_to(np.float32([0.3, 0.2, 9, 0]), (H, W, 4)).copy()
    ids = np.arange(H * W).reshape(H, W) % 3
    r = temporal_accumulate(fr, [label(ids)], [label((ids + 1) % 3)], [0.005], hist=(hc, st), var_spatial=np.full((H, W), 0.25, np.float32))
    none = temporal_accumulate(fr, [label(ids)], [label(ids)], [0.005], var_spatial=np.full((H, W), 0.25, np.float32))
    assert not r["S"].any()
    for key in ("colour", "state", "variance"):
        assert np.array_equal(r[key], none[key]), key
