"""CPU suite: tests/np_firefly.py, the float32 statement of the firefly clamp (include/mi_denoise.h, section a4l), held to a plain
per-pixel Python loop written from the header on frames of 1..6 x 1..6 with planted NaN / +-Inf / negative texels, and to answers
worked out by hand."""
import math

import numpy as np
import pytest

import np_firefly as chk
from np_albedo import widen
from np_temporal_accumulate_exact import lum32

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_but_nan(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(bits(got)[~wn], bits(want)[~wn])


def loop_clamp(frame, radius, rank, gain, floor):
    """The header, pixel by pixel: Python lists and sorted(), float32 scalars for the arithmetic."""
    C = widen(frame)
    h, w = C.shape[:2]
    with np.errstate(all="ignore"):
        L = lum32(C)
        out = C.copy()
        for y in range(h):
            for x in range(w):
                valid = [L[y + j, x + i] for j in range(-radius, radius + 1) for i in range(-radius, radius + 1)
                         if (i, j) != (0, 0) and 0 <= y + j < h and 0 <= x + i < w and math.isfinite(L[y + j, x + i])]
                if not valid:
                    continue
                m = sorted(valid, reverse=True)[min(rank, len(valid)) - 1]
                T = max(F32(gain) * F32(m), F32(floor))
                lc = L[y, x]
                if not math.isfinite(lc):
                    out[y, x, :3] = T
                elif lc > T:
                    s = F32(T) / F32(lc)
                    out[y, x, :3] = C[y, x, :3] * s
    return out


@pytest.mark.parametrize("radius", (1, 2))
def test_the_checker_is_the_per_pixel_loop(radius):
    rng = np.random.default_rng(11)
    n = 0
    for h in range(1, 7):
        for w in range(1, 7):
            f = np.exp(rng.uniform(np.log(1e-2), np.log(1e1), (h, w, 4))).astype(np.float32)
            for v in (np.nan, np.inf, -np.inf, -2.0, 4096.0):                 # planted where the frame has room, one channel each
                y, x = rng.integers(0, h), rng.integers(0, w)
                if rng.random() < 0.6:
                    f[y, x, rng.integers(0, 3)] = v
            for dt in (np.float32, np.float16, np.uint8):
                fr = rng.integers(0, 256, (h, w, 4), dtype=np.uint8) if dt == np.uint8 else f.astype(dt)
                for rank in (1, 2, 3, 4):
                    for gain, floor in ((1.0, 0.0), (1.5, 0.25)):
                        got = chk.firefly_clamp(fr, radius, rank, gain, floor)
                        assert got.dtype == np.float32 and same_but_nan(got, loop_clamp(fr, radius, rank, gain, floor)), (h, w, dt, rank, gain, floor)
                        assert np.array_equal(bits(got[..., 3]), bits(widen(fr)[..., 3])), "alpha passes through"
                        n += 1
    assert n == 36 * 3 * 4 * 2


C0 = np.float32([0.375, 0.5, 0.25, 0.75])             # a constant texel: 4096 x it and 2^-12 of that are exact


def constant(h, w):
    return np.broadcast_to(C0, (h, w, 4)).copy()


def fireflies(h, w, at):
    f = constant(h, w)
    for y, x in at:
        f[y, x, :3] *= F32(4096)
    return f


@pytest.mark.parametrize("radius", (1, 2))
def test_one_firefly_of_4096_comes_back_as_the_constant_frame(radius):
    for at in ((3, 4), (0, 0), (0, 8), (6, 0), (6, 8), (0, 3), (6, 5)):       # inside, the corners, two edges
        got = chk.firefly_clamp(fireflies(7, 9, [at]), radius, 1, 1.0, 0.0)
        assert np.array_equal(bits(got), bits(constant(7, 9))), at            # s = l / (4096 l) is exactly 2^-12


def test_a_pair_needs_rank_2_and_a_block_rank_4():
    pair, block = [(3, 4), (3, 5)], [(3, 4), (3, 5), (4, 4), (4, 5)]
    clean = constant(7, 9)
    f = fireflies(7, 9, pair)
    assert np.array_equal(bits(chk.firefly_clamp(f, 1, 1)), bits(f)), "each is the other's maximum: rank 1 leaves the pair"
    assert np.array_equal(bits(chk.firefly_clamp(f, 1, 2)), bits(clean))
    f = fireflies(7, 9, block)
    for rank in (1, 2, 3):
        assert np.array_equal(bits(chk.firefly_clamp(f, 1, rank)), bits(f)), rank
    assert np.array_equal(bits(chk.firefly_clamp(f, 1, 4)), bits(clean))
    assert np.array_equal(bits(chk.firefly_clamp(f, 2, 4)), bits(clean))


def test_fewer_valid_neighbours_than_the_rank_take_the_smallest():
    f = constant(4, 4)
    f[0, 1, :3], f[1, 0, :3], f[1, 1, :3] = C0[:3] * F32(2), C0[:3] * F32(4), C0[:3] * F32(8)     # the corner's three neighbours
    f[0, 0, :3] = C0[:3] * F32(64)
    got = chk.firefly_clamp(f, 1, 4)
    assert np.array_equal(bits(got[0, 0]), bits(np.append(C0[:3] * F32(2), C0[3]))), "n = 3 < rank 4: the third largest, 2 x"
    assert np.array_equal(bits(chk.firefly_clamp(f, 1, 2)[0, 0]), bits(np.append(C0[:3] * F32(4), C0[3])))


def test_pass_through_without_a_valid_neighbour():
    one = np.float32([[[5.0, np.nan, 1.0, 0.5]]])
    assert same_but_nan(chk.firefly_clamp(one, 2, 1), one), "1 x 1"
    f = np.full((3, 3, 4), np.nan, np.float32)
    f[1, 1] = (1e6, 2.0, 3.0, 0.25)
    got = chk.firefly_clamp(f, 1, 1)
    assert np.array_equal(bits(got[1, 1]), bits(f[1, 1])), "every neighbour NaN: the centre passes"
    f[..., 1] = np.inf
    assert same_but_nan(chk.firefly_clamp(f, 1, 1), f), "nothing valid anywhere: the frame passes"


def test_a_nan_centre_becomes_a_grey_of_the_limit():
    f = constant(5, 5)
    for ch, v in enumerate((np.nan, np.inf, -np.inf)):
        g = f.copy()
        g[2, 2, ch] = v
        g[2, 2, 3] = 0.125
        got = chk.firefly_clamp(g, 1, 1)
        T = lum32(C0[None])[0]
        assert np.array_equal(bits(got[2, 2]), bits(np.float32([T, T, T, 0.125]))), v
        g[2, 2] = f[2, 2]
        assert np.array_equal(bits(np.delete(got.reshape(-1, 4), 12, 0)), bits(np.delete(g.reshape(-1, 4), 12, 0))), "its neighbours ignore it"


def test_gain_and_floor_decide_and_a_tie_passes():
    grey = lambda v: np.float32([v, v, v, 1.0])       # l(grey v) is v up to the rounding of the three weights
    f = np.broadcast_to(grey(1.0), (3, 3, 4)).copy()
    l1 = lum32(grey(1.0)[None])[0]
    f[1, 1] = grey(1.25)
    assert np.array_equal(bits(chk.firefly_clamp(f, 1, 1, 1.5, 0.0)), bits(f)), "gain 1.5: 1.25 is let through"
    got = chk.firefly_clamp(f, 1, 1, 1.0, 0.0)[1, 1]
    lc = lum32(f[1, 1][None])[0]
    assert np.array_equal(bits(got[:3]), bits(f[1, 1, :3] * (l1 / lc))) and got[0] < 1.25, "gain 1: clamped"
    d = np.broadcast_to(grey(0.0625), (3, 3, 4)).copy()
    d[1, 1] = grey(0.2)
    assert np.array_equal(bits(chk.firefly_clamp(d, 1, 1, 1.0, 0.25)), bits(d)), "floor 0.25: 0.2 is let through"
    assert chk.firefly_clamp(d, 1, 1, 1.0, 0.0)[1, 1, 0] < 0.1, "floor 0: clamped"
    tie = constant(3, 3)
    assert np.array_equal(bits(chk.firefly_clamp(tie, 1, 1, 1.0, 0.0)), bits(tie)), "lc == T everywhere: unchanged"
    c = {}
    chk.firefly_clamp(tie, 1, 1, 1.0, 0.0, counts=c)
    assert c == dict(clamped=0, repaired=0, untouched=9, pixels=9)


def test_negative_luminance_is_valid_and_the_limit_is_never_negative():
    f = constant(3, 3)
    f[..., :3] = -1.0
    f[1, 1, :3] = 0.5
    got = chk.firefly_clamp(f, 1, 1, 1.0, 0.0)
    assert np.array_equal(bits(got[1, 1, :3]), bits(np.float32([0, 0, 0]))), "T = fmaxf(gain * m, 0) = 0: s = 0"
    assert np.array_equal(bits(np.delete(got.reshape(-1, 4), 4, 0)), bits(np.delete(f.reshape(-1, 4), 4, 0)))
