"""The float64 checker of the guided filter (tests/np_guided.py) against statements that share nothing with it: a per-pixel double
loop written from the header, scipy's uniform_filter on the interior, and answers worked out by hand.  No GPU."""
import numpy as np
import pytest

import np_guided


def loop_guided(frame, guide, r, eps):
    """Section a4o, literally: per window the valid texels are gathered and the moments taken over them; per pixel the models of
    its window are averaged."""
    P = np_guided.widen(frame)
    G = P if guide is None else np_guided.widen(guide)
    h, w = P.shape[:2]
    eps = float(np.float32(eps))
    valid = np.isfinite(P[..., :3]).all(-1) & np.isfinite(G[..., :3]).all(-1)
    a, b, model = np.zeros((h, w, 3, 3)), np.zeros((h, w, 3)), np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            ys, xs = slice(max(0, y - r), min(h, y + r + 1)), slice(max(0, x - r), min(w, x + r + 1))
            ok = valid[ys, xs]
            if not ok.any():
                continue
            I, p = G[ys, xs, :3][ok], P[ys, xs, :3][ok]
            mu, nu = I.mean(0), p.mean(0)
            Sig = (I[:, :, None] * I[:, None, :]).mean(0) - np.outer(mu, mu)
            C = (I[:, :, None] * p[:, None, :]).mean(0) - np.outer(mu, nu)
            a[y, x] = np.linalg.inv(Sig + eps * np.eye(3)) @ C
            b[y, x] = nu - a[y, x].T @ mu
            model[y, x] = True
    out, T = P.copy(), np.full((h, w, 3), np.nan)
    for y in range(h):
        for x in range(w):
            ys, xs = slice(max(0, y - r), min(h, y + r + 1)), slice(max(0, x - r), min(w, x + r + 1))
            ok = model[ys, xs]
            if not (valid[y, x] and ok.any()):
                continue
            ab, bb = a[ys, xs][ok].mean(0), b[ys, xs][ok].mean(0)
            out[y, x, :3] = ab.T @ G[y, x, :3] + bb
            T[y, x] = np.abs(a[ys, xs][ok]).mean(0).T @ np.abs(G[y, x, :3]) + np.abs(b[ys, xs][ok]).mean(0)
    return out, T


def _frames(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.random((h, w, 4)).astype(np.float32), rng.random((h, w, 4)).astype(np.float32)


def _close(got, want, scale):
    both_nan = np.isnan(got) & np.isnan(want)
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    d = np.abs(np.where(both_nan | inf, 0.0, got - want))
    assert not np.isnan(d).any()
    assert float((d / scale).max()) < 1e-9


@pytest.mark.parametrize("plant", ["none", "in", "guide", "both"])
def test_against_the_double_loop(plant):
    for i, (h, w) in enumerate([(1, 1), (1, 5), (2, 3), (5, 1), (7, 9), (13, 13), (4, 11)]):
        for r in range(1, 8):
            p, g = _frames(h, w, 100 * i + r)
            rng = np.random.default_rng(7 * i + r)
            for img, on in ((p, plant in ("in", "both")), (g, plant in ("guide", "both"))):
                if on:
                    for bad in (np.nan, np.inf, -np.inf):
                        img[rng.integers(h), rng.integers(w), rng.integers(3)] = bad
            for guide in (g, None):
                ref = np_guided.guided(p, guide, r, 1e-2)
                out, T = loop_guided(p, guide, r, 1e-2)
                scale = np.maximum(1.0, np.nan_to_num(ref["T"], nan=1.0, posinf=1.0))
                _close(ref["out"][..., :3], out[..., :3], scale)
                np.testing.assert_array_equal(ref["out"][..., 3], out[..., 3])
                f = ref["filtered"]
                assert np.array_equal(f, ~np.isnan(T).any(-1))
                assert float(np.abs(ref["T"][f] - T[f]).max(initial=0.0)) < 1e-9 * max(1.0, float(T[f].max(initial=0.0)))


def test_against_scipy_on_the_interior():
    ndimage = pytest.importorskip("scipy.ndimage")
    h, w, r, eps = 40, 53, 3, np.float32(1e-2)
    p, g = _frames(h, w, 3)
    P, G = p.astype(np.float64)[..., :3], g.astype(np.float64)[..., :3]
    box = lambda x: ndimage.uniform_filter(x, size=(2 * r + 1, 2 * r + 1) + (1,) * (x.ndim - 2), mode="constant")
    mu, nu = box(G), box(P)
    Sig = box(G[..., :, None] * G[..., None, :]) - mu[..., :, None] * mu[..., None, :]
    C = box(G[..., :, None] * P[..., None, :]) - mu[..., :, None] * nu[..., None, :]
    a = np.linalg.solve(Sig + float(eps) * np.eye(3), C)
    b = nu - np.einsum("hwjc,hwj->hwc", a, mu)
    out = np.einsum("hwjc,hwj->hwc", box(a), G) + box(b)
    ref = np_guided.guided(p, g, r, eps)
    m = 2 * r                                           # the models of the window are themselves interior
    assert float(np.abs(ref["out"][m:-m, m:-m, :3] - out[m:-m, m:-m]).max()) < 1e-10


def test_constant_guide_gives_the_box_mean_of_the_box_mean():
    h, w, r = 9, 14, 2
    p, _ = _frames(h, w, 5)
    g = np.full((h, w, 4), 0.37, np.float32)
    ref = np_guided.guided(p, g, r, 1e-3)
    assert float(np.abs(ref["abar"]).max()) < 1e-12 and float(ref["lam_max"].max()) < 1e-12
    n = np_guided.box_sum(np.ones((h, w)), r)
    mean = np_guided.box_sum(p.astype(np.float64)[..., :3], r) / n[..., None]
    want = np_guided.box_sum(mean, r) / n[..., None]
    assert float(np.abs(ref["out"][..., :3] - want).max()) < 1e-12


def test_grey_guide_on_itself():
    """I = (g, g, g), p = I.  In a window with variance s2 of g: Sigma = s2 J (J all ones), C = s2 J.  (s2 J + eps U)^-1 =
    (U - s2 J / (3 s2 + eps)) / eps (Sherman-Morrison, J J = 3 J), so a = s2 J (U - s2 J / (3 s2 + eps)) / eps
    = s2 J (3 s2 + eps - 3 s2) / (eps (3 s2 + eps)) = J s2 / (3 s2 + eps): every a_jc = s2 / (3 s2 + eps)."""
    h, w, r, eps = 11, 12, 2, np.float32(1e-2)
    rng = np.random.default_rng(2)
    g1 = rng.random((h, w)).astype(np.float32)
    img = np.stack([g1, g1, g1, np.ones_like(g1)], -1)
    ref = np_guided.guided(img, None, r, eps)
    n = np_guided.box_sum(np.ones((h, w)), r)
    G = g1.astype(np.float64)
    s2 = np_guided.box_sum(G * G, r) / n - (np_guided.box_sum(G, r) / n) ** 2
    want = s2 / (3 * s2 + float(eps))
    assert float(np.abs(ref["a"] - want[..., None, None]).max()) < 1e-12
    assert float(np.abs(ref["lam_max"] - 3 * s2).max()) < 1e-12


def test_an_exact_affine_frame_comes_back():
    """p = A^T I + beta in numbers that fp32 holds exactly (sixteenths in the guide, quarters in A, eighths in beta), on white noise:
    the covariance of every window is far from singular, so with eps = 1e-12 the fit is the frame."""
    h, w, r = 15, 17, 3
    rng = np.random.default_rng(9)
    g = np.ones((h, w, 4), np.float32)
    g[..., :3] = rng.integers(0, 17, (h, w, 3)) / 16.0
    A, beta = rng.integers(-8, 9, (3, 3)) / 4.0, rng.integers(-8, 9, 3) / 8.0
    p = np.ones((h, w, 4))
    p[..., :3] = g[..., :3].astype(np.float64) @ A + beta
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p)
    ref = np_guided.guided(p32, g, r, 1e-12)
    assert float(ref["lam_max"].min()) > 1e-2
    assert float(np.abs(ref["out"][..., :3] - p[..., :3]).max()) < 1e-9
    assert float(np.abs(ref["abar"] - A).max()) < 1e-9


def test_nothing_valid_around_a_pixel_passes_it_through():
    h, w, r = 9, 9, 1
    p, g = _frames(h, w, 4)
    g[2:7, 2:7, 1] = np.nan                            # a 5 x 5 hole: the windows of its inner 3 x 3 hold no valid texel
    ref = np_guided.guided(p, g, r, 1e-2)
    assert not ref["model"][3:6, 3:6].any() and ref["model"][2, 2]
    assert not ref["filtered"][2:7, 2:7].any()
    np.testing.assert_array_equal(ref["out"][2:7, 2:7], p.astype(np.float64)[2:7, 2:7])
    # and a valid pixel whose whole window has no model: an island inside an invalid sea of radius 2 r
    g2 = np.full((h, w, 4), np.nan, np.float32)
    g2[4, 4] = 0.5
    ref = np_guided.guided(p, g2, r, 1e-2)
    assert ref["valid"][4, 4] and ref["filtered"][4, 4]          # its own window holds itself: m = 1
    p3 = p.copy()
    p3[...] = np.nan
    ref = np_guided.guided(p3, None, r, 1e-2)
    assert not ref["model"].any() and not ref["filtered"].any() and np.isnan(ref["out"][..., :3]).all()
