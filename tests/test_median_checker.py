"""CPU suite: the float64 checker of the median filters (tests/np_median.py, section a4p) held to a per-pixel loop written from the
definition (rank counting, no sort), to scipy.ndimage.median_filter on the interior, and to answers worked out by hand."""
import numpy as np
import pytest

import np_median
from np_albedo import widen

F32 = np.float32


def loop_median(frame, layers, sigmas, radius):
    """The definition, pixel by pixel: (out, margin)."""
    C = widen(frame).astype(np.float64)
    h, w = C.shape[:2]
    G = [(widen(l)[..., :3] * np_median.scale_of(s)).astype(F32).astype(np.float64) for l, s in zip(layers, sigmas)]
    out = C.copy()
    margin = np.full((h, w, 3), np.inf)
    for y in range(h):
        for x in range(w):
            taps = [(yy, xx) for yy in range(y - radius, y + radius + 1) for xx in range(x - radius, x + radius + 1) if 0 <= yy < h and 0 <= xx < w]
            wts = []
            for yy, xx in taps:
                arg = 0.0
                with np.errstate(all="ignore"):
                    for g in G:
                        arg -= float(((g[y, x] - g[yy, xx]) ** 2).sum())
                wt = 2.0 ** arg if np.isfinite(arg) and arg >= -126 else 0.0
                wts.append(wt if G else 1.0)
            for c in range(3):
                V = [(C[yy, xx, c], wt) for (yy, xx), wt in zip(taps, wts) if np.isfinite(C[yy, xx, c]) and wt > 0]
                if not V:
                    continue
                W = sum(wt for _, wt in V)
                best = None
                for v, _ in V:
                    s_le = sum(wt for u, wt in V if u <= v)
                    if 2 * s_le >= W and (best is None or v < best):
                        best = v
                out[y, x, c] = best
                s_le = sum(wt for u, wt in V if u <= best)
                s_lt = sum(wt for u, wt in V if u < best)
                margin[y, x, c] = min(s_le - W / 2, W / 2 - s_lt) / W
    return out.astype(F32), margin


def random_case(rng, h, w, bad_frame, bad_guide, n_layers):
    frame = rng.random((h, w, 4)).astype(F32)
    frame[..., :3] = np.round(frame[..., :3] * 8) / 8               # ties on purpose
    layers = [(rng.integers(0, 3, (h, w, 4)) * 0.05 + rng.random((h, w, 4)) * 0.01).astype(F32) for _ in range(n_layers)]
    bads = F32([np.nan, np.inf, -np.inf])
    if bad_frame:
        m = rng.random((h, w, 3)) < 0.2
        frame[..., :3][m] = rng.choice(bads, int(m.sum()))
    if bad_guide and layers:
        m = rng.random((h, w, 3)) < 0.1
        layers[0][..., :3][m] = rng.choice(bads, int(m.sum()))
    return frame, layers, [0.05] * n_layers


@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("bad", ("none", "frame", "guide", "both"))
def test_against_the_definition_loop(radius, bad):
    rng = np.random.default_rng(radius * 10 + len(bad))
    for n in range(1, 10):
        for n_layers in (0, 1, 2):
            frame, layers, sigmas = random_case(rng, n, 10 - n if n % 2 else n, bad in ("frame", "both"), bad in ("guide", "both"), n_layers)
            out, margin, _ = np_median.median(frame, layers, sigmas, radius)
            want, want_margin = loop_median(frame, layers, sigmas, radius)
            assert np_median.same_values(out[..., :3], want[..., :3]).all()
            assert np_median.same_values(out[..., 3], frame[..., 3]).all()
            fin = np.isfinite(want_margin)
            assert np.array_equal(fin, np.isfinite(margin))
            assert np.allclose(margin[fin], want_margin[fin], rtol=0, atol=1e-12)


@pytest.mark.parametrize("radius", (1, 2, 3))
def test_plain_median_against_scipy_on_the_interior(radius):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(radius)
    frame = rng.random((23, 31, 4)).astype(F32)
    out, margin, exact = np_median.median(frame, None, None, radius)
    r = radius
    for c in range(3):
        want = ndimage.median_filter(frame[..., c], size=2 * r + 1)
        assert np.array_equal(out[r:-r, r:-r, c], want[r:-r, r:-r])
    assert exact.all() and (margin[r:-r, r:-r] > 0).all()        # (a cut window of even count may tie exactly: margin 0, both sides exact)


def test_hand_answers():
    const = np.full((7, 9, 4), 0.375, F32)
    for r in (1, 2, 3):
        assert np.array_equal(np_median.median(const, None, None, r)[0], const)
    step = np.zeros((9, 12, 4), F32)
    step[:, 6:] = 1.0
    for r in (1, 2, 3):                                         # a straight edge: more than half of every window lies on the pixel's side
        assert np.array_equal(np_median.median(step, None, None, r)[0], step)
    impulse = np.full((9, 9, 4), 0.25, F32)
    impulse[4, 4, :3] = 50.0
    for r in (1, 2, 3):
        assert np.array_equal(np_median.median(impulse, None, None, r)[0][..., :3], np.full((9, 9, 3), 0.25, F32))


def test_two_valued_guide_gives_the_plain_median_of_the_own_region():
    rng = np.random.default_rng(5)
    h, w, r = 8, 10, 2
    frame = rng.random((h, w, 4)).astype(F32)
    guide = np.zeros((h, w, 4), F32)
    guide[:, 5:] = 1.0
    out, margin, exact = np_median.median(frame, [guide], [0.01], r)           # arg = -7213 across: the weight underflows to exactly 0
    assert exact.all()
    for half in (slice(0, 5), slice(5, w)):
        own = np_median.median(frame[:, half], None, None, r)[0]
        assert np.array_equal(out[:, half], own)


def test_nan_centre_and_all_nan_frame():
    frame = np.arange(25 * 4, dtype=F32).reshape(5, 5, 4)
    frame[2, 2, 0] = np.nan
    out = np_median.median(frame, None, None, 1)[0]
    neighbours = np.sort(np.delete(frame[1:4, 1:4, 0].ravel(), 4))
    assert out[2, 2, 0] == neighbours[3]                       # eight valid taps: the lower median is the fourth
    assert out[2, 2, 1] == frame[2, 2, 1]
    nothing = np.full((4, 6, 4), np.nan, F32)
    nothing[..., 3] = 0.5
    got, margin, _ = np_median.median(nothing, None, None, 2)
    assert np_median.same_values(got, nothing).all() and np.isinf(margin).all()
