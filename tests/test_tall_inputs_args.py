"""The recipe of the tall-frame and later-tile GPU tests (tests/tall_inputs.py) held to its conditions with the checkers alone: no
kernel takes part.

For every filter those tests run, the existing checker runs on a frame of five periods more than the small frame.  Its interior rows
repeat with period 37 to the last bit, and -- the same property with the edges included -- the whole output is the small frame's
output indexed by row_map.  The exact constructions reused there stay exact on the tiled frames.
"""
import numpy as np
import pytest

import firefly_inputs
import median_inputs as mi
import np_firefly
import np_median
import oracle
import tall_inputs as ti

MORE = 5 * ti.PERIOD


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def holds(run, patterns, r, H):
    """run(frames of h rows) -> list of arrays [h, ...]: checked on hs and on hs + MORE rows."""
    hs = ti.small_height(H, r)
    small, medium = run(ti.tiled(patterns, hs)), run(ti.tiled(patterns, hs + MORE))
    rows = ti.row_map(hs + MORE, r, hs)
    for s, m in zip(small, medium):
        assert ti.interior_repeats(m, r)
        assert np.array_equal(bits(m), bits(np.asarray(s)[rows]))
    return small


def test_heights_and_the_row_map():
    assert ti.cdiv(ti.H4, 4) == ti.GRID_Y == ti.cdiv(ti.H16, 16) and ti.GRID_Y > 65536
    assert (4 * 65536) % ti.PERIOD == 36 and (16 * 65536) % ti.PERIOD == 33          # a wrapped block index lands on another phase
    for H in (ti.H4, ti.H16):
        for r in (1, 2, 3, 4, 18):
            hs = ti.small_height(H, r)
            assert ti.PERIOD + 2 * r <= hs < 2 * ti.PERIOD + 2 * r and hs % ti.PERIOD == H % ti.PERIOD
            rows = ti.row_map(H, r, hs)
            y = np.arange(H)
            assert np.array_equal(rows % ti.PERIOD, y % ti.PERIOD), "the same phase"
            assert np.array_equal(np.minimum(rows, r), np.minimum(y, r)), "the same distance to the top edge, up to the reach"
            assert np.array_equal(np.minimum(hs - 1 - rows, r), np.minimum(H - 1 - y, r)), "and to the bottom edge"
            assert rows.min() == 0 and rows.max() == hs - 1 and len(np.unique(rows)) == ti.PERIOD + 2 * r, "both edges and one whole period"


@pytest.mark.parametrize("w", ti.WIDTHS)
@pytest.mark.parametrize("clip", (False, True))
def test_accumulation_repeats_and_stays_exact(w, clip):
    pat = ti.accumulate_patterns(w)
    assert ti.distinct_rows(pat["frame"])
    mv = pat["motion"]
    assert np.abs(mv[..., 1]).max() == 3 and np.array_equal(mv * 2, np.round(mv * 2)), "motion crosses rows, in integers and halves"
    assert np.abs(mv).max() + 1 <= ti.ACCUM_REACH
    colour, state, vt = holds(lambda t: ti.accumulate_answer(t, clip), pat, ti.ACCUM_REACH, ti.H4)      # (asserts its sums exact itself)
    if clip:
        plain = ti.accumulate_answer(ti.tiled(pat, ti.small_height(ti.H4, ti.ACCUM_REACH)), False)
        assert not np.array_equal(plain[0], colour), "the box clips something"


@pytest.mark.parametrize("w", ti.WIDTHS)
@pytest.mark.parametrize("L", (1, 5))
def test_atrous_pass_repeats_and_stays_exact(w, L):
    pat = ti.atrous_patterns(w, L)
    assert ti.distinct_rows(pat["frame"])
    shares = []

    def run(t):
        out, share = ti.atrous_answer(t)
        shares.append(share)
        return [out]
    holds(run, pat, ti.ATROUS_REACH, ti.H4)
    assert all(0.02 < s < 0.98 for s in shares), shares


@pytest.mark.parametrize("w", ti.WIDTHS)
def test_variance_pass_and_temporal_pass_repeat_and_stay_exact(w):
    shares = []

    def variance(t):
        out, share = ti.variance_answer(t)
        shares.append(share)
        return list(out)

    def temporal(t):
        out, share = ti.temporal_answer(t)
        shares.append(share)
        return [out]
    pat = ti.variance_patterns(w, 5)
    assert ti.distinct_rows(np.concatenate([pat["frame"], pat["variance"][..., None]], -1))
    holds(variance, pat, ti.ATROUS_REACH, ti.H4)
    pat = ti.temporal_patterns(w, 5)
    assert all(ti.distinct_rows(pat[f"frame{f}"]) for f in range(ti.TEMPORAL_FRAMES))
    holds(temporal, pat, ti.ATROUS_REACH, ti.H4)
    assert all(0.02 < s < 0.98 for s in shares), shares


@pytest.mark.parametrize("w", ti.WIDTHS)
def test_moments_repeat(w):
    pat = ti.moments_patterns(w, 5)
    assert ti.distinct_rows(pat["frame1"])
    holds(lambda t: list(ti.moments_reference(t, 5)), pat, ti.MOMENTS_REACH, ti.H4)


@pytest.mark.parametrize("w", ti.WIDTHS)
@pytest.mark.parametrize("radius", mi.RADII)
def test_median_repeats_and_stays_exact(w, radius):
    pat = ti.median_patterns(w)
    assert ti.distinct_rows(pat["frame"])

    def run(t):
        out, _, exact = np_median.median(t["frame"], [t["guide"]] + [np.zeros_like(t["guide"])] * 4, [mi.EXACT_SIGMA] * 5, radius)
        assert exact.all()
        one = np_median.median(t["frame"], [t["guide"]], [mi.EXACT_SIGMA], radius)[0]
        assert np_median.same_values(out, one).all(), "all-zero layers change no weight"
        return [out]
    (out,) = holds(run, pat, radius, ti.H4)
    hs = out.shape[0]
    assert not np_median.same_values(out, np_median.median(ti.tile_rows(pat["frame"], hs), None, None, radius)[0]).all(), "the guide decides something"


@pytest.mark.parametrize("radius", mi.RADII)
def test_tie_frame_medians_repeat(radius):
    w = 192
    hs = ti.small_height(10944, radius)
    fr, more = ti.tie_frame(hs, w), ti.tie_frame(hs + MORE, w)
    assert np.isfinite(fr).all() and np.array_equal(fr * 16, np.round(fr * 16))
    assert len(np.unique(fr[..., 0])) < fr[..., 0].size / 20, "many tied values"
    assert ti.distinct_rows(fr[:ti.PERIOD])
    small, medium = np_median.median(fr, None, None, radius)[0], np_median.median(more, None, None, radius)[0]
    assert ti.interior_repeats(medium, radius)
    assert np.array_equal(bits(medium), bits(small[ti.row_map(hs + MORE, radius, hs)]))


def test_firefly_clamp_repeats():
    w, radius, rank = 192, 2, 2
    pat = dict(frame=firefly_inputs.frame_of((ti.PERIOD, w), np.float32, seed=1))
    assert ti.distinct_rows(pat["frame"])
    holds(lambda t: [np_firefly.firefly_clamp(t["frame"], radius, rank)], pat, radius, 16 * 1367)


def test_bilateral_checkers_repeat():
    w = 3
    pat = ti.bilateral_patterns(w)
    assert ti.distinct_rows(pat["frame"])
    ss, sc = ti.BILATERAL_SIGMAS

    def layers(t):
        W = np.zeros(t["frame"].shape[:2] + (8,), np.float32)
        for lay in t["layers"]:
            W = oracle.bilateral_layers_accum(t["frame"], lay, W, ti.BILATERAL_GENERIC_RADIUS, ss, sc)
        return [oracle.normalize(W)]
    holds(layers, pat, ti.BILATERAL_GENERIC_RADIUS, ti.H16)
    holds(lambda t: [oracle.bilateral_texture(t["frame"], ti.BILATERAL_TUNED_RADIUS, ss, sc)], pat, ti.BILATERAL_TUNED_RADIUS, ti.H16)


def test_joint_and_temporal_bilateral_checkers_repeat():
    import np_bilateral_joint
    import np_bilateral_temporal
    w = 3
    ss, sc = ti.BILATERAL_SIGMAS
    L, r = ti.BILATERAL_JOINT_LAYERS, ti.BILATERAL_JOINT_RADIUS
    holds(lambda t: np_bilateral_joint.bilateral_joint([t["frame"]], [t["layers"]], [sc] * L, 0, r, ss), ti.bilateral_patterns(w, n_layers=L), r, ti.H16)
    pat = ti.bilateral_pair_patterns(w)
    assert not np.array_equal(pat["frame0"], pat["frame1"])
    r = ti.BILATERAL_GENERIC_RADIUS
    holds(lambda t: [np.asarray(o) for o in np_bilateral_temporal.bilateral_temporal([t["frame0"], t["frame1"]], 1, r, ss, sc, layers=[t["layers0"], t["layers1"]],
                                                                                      first=0, count=1)], pat, r, ti.H16)


def test_nlm_oracle_repeats():
    search, patch, r = (-1, 2), (0, 2), 2
    pat = {"frame": ti.bilateral_patterns(3)["frame"]}

    def run(t):
        fr = t["frame"]
        return [oracle.normalize(oracle.nlm_accum(fr, fr, np.zeros(fr.shape[:2] + (8,), np.float32), 0.5, search=search, patch=patch))]
    holds(run, pat, r, ti.H16)


@pytest.mark.parametrize("radius", (1, 16))
def test_guided_checker_repeats_far_below_its_bound(radius):
    """np_guided sums cumulatively, so its interior repeats up to float64 rounding only: 2^-20 of the header's bound is asserted, and
    the GPU test compares under the bound itself."""
    import guided_inputs as gdi
    import np_guided
    w, reach = 3, 2 * radius
    noisy, alb, _ = gdi.scene(ti.PERIOD, w, radius)
    hs = ti.small_height(524800, reach)
    small = np_guided.guided(ti.tile_rows(noisy, hs), ti.tile_rows(alb, hs), radius, gdi.EPS)
    medium = np_guided.guided(ti.tile_rows(noisy, hs + MORE), ti.tile_rows(alb, hs + MORE), radius, gdi.EPS)
    assert small["filtered"].all() and medium["filtered"].all()
    rows = ti.row_map(hs + MORE, reach, hs)
    tol = np_guided.tolerance(medium)
    assert (np.abs(medium["out"][..., :3] - small["out"][rows][..., :3]) <= 2.0 ** -20 * tol).all()
    assert (np.abs(tol - np_guided.tolerance(small)[rows]) <= 2.0 ** -20 * tol).all()


def test_layer_guided_nlm_checkers_repeat():
    import np_nlm_joint
    import np_nlm_layers
    import np_nlm_layers_temporal
    search, patch, r = (-1, 2), (0, 2), 2
    pat = ti.bilateral_pair_patterns(3)
    fr = lambda t: [t["frame0"], t["frame1"]]
    ly = lambda t: [t["layers0"], t["layers1"]]
    holds(lambda t: [np_nlm_layers.nlm_layers(t["frame0"], t["layers0"], 0.5, search, patch)], pat, r, ti.H16)
    holds(lambda t: np_nlm_layers_temporal.nlm_layers_temporal(fr(t), ly(t), 1, 0.5, search, patch, first=0, count=1), pat, r, ti.H16)
    holds(lambda t: np_nlm_joint.nlm_joint(fr(t), ly(t), [0.5, 0.8], 1, search, patch, first=0, count=1), pat, r, ti.H16)


def test_colour_box_and_image_metrics_checkers_repeat():
    import np_color_bounds
    import np_image_metrics as npm
    rng = np.random.default_rng(12)
    pat = dict(frame=rng.integers(0, 256, (ti.PERIOD, 67, 4)).astype(np.float32))
    pat["frame"][5, 30, 0] = np.nan
    for radius, gamma in ((1, 0.0), (2, 2.5)):
        with np.errstate(invalid="ignore"):
            lo, hi = holds(lambda t: list(np_color_bounds.color_bounds(t["frame"], radius, gamma)), pat, radius, 21904)
        if gamma == 0.0:
            fin = np.isfinite(lo[..., :3])
            assert np.array_equal(lo, hi) and np.array_equal(lo[..., :3][fin], lo[..., :3][fin].astype(np.float32)), "lo = hi = mu, a float32"
    a = rng.integers(0, 16, (ti.PERIOD, 67, 4)).astype(np.float32)
    b = np.clip(a + rng.integers(-2, 3, a.shape), 0, 15).astype(np.float32)
    a[9, 40, 1] = np.nan
    run = lambda t: (lambda r: [np.nan_to_num(r["map"], nan=-9.0), r["M"]])(npm.image_metrics(t["a"], t["b"], peak=16.0, eps=1e-2))
    holds(run, dict(a=a, b=b), npm.R, 43712)
    whole = npm.image_metrics(ti.tile_rows(a, 3 * ti.PERIOD + 15), ti.tile_rows(b, 3 * ti.PERIOD + 15), ssim=False)["sums"]
    per, rem = npm.image_metrics(a, b, ssim=False)["sums"], npm.image_metrics(a[:15], b[:15], ssim=False)["sums"]
    for i in (npm.I_VALID, npm.I_INVALID, *range(npm.I_SQ, npm.I_SQ + 3), *range(npm.I_ABS, npm.I_ABS + 3)):
        assert whole[i] == 3 * per[i] + rem[i], "integer sums: exact, and additive over rows"
    assert whole[npm.I_MAX] == max(per[npm.I_MAX], rem[npm.I_MAX])


def test_later_tiles_geometry():
    for cu in (64, 256, 304):
        for per_cu in (4, 8):
            cap = cu * per_cu
            h = ti.later_tiles_height(cap, 3)
            tiles = 3 * ti.cdiv(h, 16)
            assert tiles >= 2 * cap + 3 and ti.rounds_of(tiles, cap) >= 3 and h % 16 == 0
    assert ti.later_tiles_height(4 * 256, 3) == 10944
