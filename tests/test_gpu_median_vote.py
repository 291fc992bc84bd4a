"""GPU suite: the vote of the plain selection class of mid_median_filter (section a4p; no layers, radius 1, 2 and 3): a workgroup
takes the selection network -- 9, 25 or 49 inputs -- only when every texel of its LDS tile is inside the image with finite r, g, b.

A 50 x 200 frame has 4 x 4 tiles of 64 x 16, of which the four in the middle see no border at any radius.  A single NaN, and a single
Inf, planted at a texel that lies in exactly ONE workgroup's LDS tile flips exactly that workgroup's vote: every pixel outside the
planted texel's window keeps the bits of the unplanted run, the pixels inside match the checker.  The border: a 48 x 192 frame, 3 x 3
tiles, where only the centre tile votes yes, and the same frame one texel smaller and larger each way; both against the checker, every
pixel.  And the network against rank counting on the same frame: one all-zero layer sends every tile to the general class."""
import numpy as np
import pytest

import median_inputs as mi
import np_median

pytestmark = pytest.mark.gpu
H, W = 50, 200
SPOT = (24, 100)                       # inside tile (1, 1), whose LDS tile covers x 64 - r .. 127 + r and y 16 - r .. 31 + r and no other tile's does


def finite_frame(h, w, seed):
    frame = mi.scene(h, w, seed=seed)[0]
    assert np.isfinite(frame).all()
    return frame


@pytest.mark.parametrize("radius", mi.RADII)
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf), ids=("nan", "inf", "-inf"))
@pytest.mark.parametrize("channel", (0, 1, 2))
def test_one_odd_texel_flips_one_workgroup(ctx, bad, channel, radius):
    r = radius
    frame = finite_frame(H, W, 11)
    base = ctx.median_filter(frame, None, None, r)
    assert np_median.same_values(base, np_median.median(frame, None, None, r)[0]).all()
    y, x = SPOT
    assert 64 + r <= x < 128 - r and 16 + r <= y < 32 - r                      # not in a neighbour's halo
    planted = frame.copy()
    planted[y, x, channel] = bad
    got = ctx.median_filter(planted, None, None, r)
    want = np_median.median(planted, None, None, r)[0]
    window = np.zeros((H, W), bool)
    window[y - r:y + r + 1, x - r:x + r + 1] = True
    assert np.array_equal(got[~window].view(np.uint32), base[~window].view(np.uint32))
    assert np_median.same_values(got[window], want[window]).all()
    assert np.isfinite(got[..., :3]).all()                                      # the odd texel itself is repaired from its neighbours


@pytest.mark.parametrize("radius", mi.RADII)
@pytest.mark.parametrize("shape", ((48, 192), (47, 191), (49, 193)), ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_border_of_the_frame(ctx, shape, radius):
    frame = finite_frame(*shape, 12)
    got = ctx.median_filter(frame, None, None, radius)
    assert np_median.same_values(got, np_median.median(frame, None, None, radius)[0]).all()


@pytest.mark.parametrize("radius", mi.RADII)
def test_the_network_against_rank_counting(ctx, radius):
    frame = finite_frame(H, W, 13)
    frame[..., :3] = np.round(frame[..., :3] * 16) / 16                         # many equal values: ties inside every window
    net = ctx.median_filter(frame, None, None, radius)
    ranks = ctx.median_filter(frame, [np.zeros((H, W, 4), np.uint8)], [0.1], radius)
    assert np_median.same_values(net, ranks).all()
    assert np_median.same_values(net, np_median.median(frame, None, None, radius)[0]).all()
