"""CPU suite: the exact answers of the recursive temporal accumulation (tests/np_temporal_accumulate_exact.py) against plain loops
over pixels and taps in rational arithmetic, every fp32 operation of section a4j rounded once by hand -- and against the float64
checker, which they must meet to its last bits or so."""
from fractions import Fraction

import numpy as np
import pytest

import np_temporal_accumulate_exact as ex
from np_temporal_accumulate import temporal_accumulate


def rnd32(x):
    """The fp32 nearest a rational (ties to even), as a Fraction; the values here are far from the subnormal range."""
    x = Fraction(x)
    if x == 0:
        return x
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = 0
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    ulp = Fraction(2) ** (e - 23)
    n, rem = divmod(x, ulp)
    rem /= ulp
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * n * ulp


def F(v):
    return Fraction(float(v))


def plain_loops(frame, layers, prev_layers, hist, mv, alpha, alpha_moments, history_max):
    h, w = frame.shape[:2]
    col, st, vt = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
    alpha, alpha_moments, history_max = F(np.float32(alpha)), F(np.float32(alpha_moments)), F(np.float32(history_max))
    lr, lg, lb = F(ex.LR), F(ex.LG), F(ex.LB)
    for y in range(h):
        for x in range(w):
            ppx, ppy = F(x) + F(mv[y, x, 0]), F(y) + F(mv[y, x, 1])
            S, hc, hs = Fraction(0), [Fraction(0)] * 4, [Fraction(0)] * 3
            if -1 < ppx < w and -1 < ppy < h:
                x0, y0 = ppx.__floor__(), ppy.__floor__()
                fx, fy = ppx - x0, ppy - y0
                for b in (0, 1):
                    for a in (0, 1):
                        qx, qy = x0 + a, y0 + b
                        bw = (fx if a else 1 - fx) * (fy if b else 1 - fy)
                        if not (0 <= qx < w and 0 <= qy < h) or bw == 0:
                            continue
                        if any((gc[y, x, :3] != gp[qy, qx, :3]).any() for gc, gp in zip(layers, prev_layers)):
                            continue
                        S += bw
                        hc = [acc + bw * F(v) for acc, v in zip(hc, hist[0][qy, qx])]
                        hs = [acc + bw * F(v) for acc, v in zip(hs, hist[1][qy, qx, :3])]
            if S > 0:
                hc = [rnd32(v / S) for v in hc]
                h1, h2 = rnd32(hs[0] / S), rnd32(hs[1] / S)
            else:
                hc, h1, h2 = [Fraction(0)] * 4, Fraction(0), Fraction(0)
            N = min(history_max, rnd32(hs[2] + 1))
            inv = rnd32(1 / N)
            al, am = max(inv, alpha), max(inv, alpha_moments)
            C = [F(v) for v in frame[y, x]]
            col[y, x] = [float(rnd32(al * rnd32(c - k) + k)) for c, k in zip(C, hc)]
            l = rnd32(lb * C[2] + rnd32(lg * C[1] + rnd32(lr * C[0])))
            m1 = rnd32(am * rnd32(l - h1) + h1)
            m2 = rnd32(am * rnd32(rnd32(l * l) - h2) + h2)
            v = rnd32(-m1 * m1 + m2)
            st[y, x] = [float(m1), float(m2), float(N), 0.0]
            vt[y, x] = float(max(v, 0))
    return col, st, vt


@pytest.mark.parametrize("L,shape", [(1, (9, 13)), (3, (17, 21)), (5, (10, 35))])
def test_exact_answers_against_plain_loops_and_the_float64_checker(L, shape):
    fr, hist, mv = ex.grey_frame(shape, 1), ex.history(shape, 1), ex.motion(shape, 1)
    ly, pl = ex.label_layers(shape, L, 1), ex.label_layers(shape, L, 0)
    col, st, vt, rejected = ex.temporal_accumulate_exact(fr, ly, pl, hist, mv, 0.0625, 0.1, 32)
    want = plain_loops(fr, ly, pl, hist, mv, 0.0625, 0.1, 32)
    for got, ref, what in zip((col, st, vt), want, ("colour", "state", "Vt")):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what
    if L <= 3:
        assert 0.05 < rejected < 0.95, rejected
    r = temporal_accumulate(fr, ly, pl, [ex.SIGMA] * L, hist=hist, motion=mv, alpha=0.0625, alpha_moments=0.1, history_max=32)
    np.testing.assert_allclose(col, r["colour"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(st, r["state"], rtol=1e-6, atol=2e-4)          # (m2 of about 1e3 to 6e4: fp32 rounding of l l)
    assert len(np.unique(st[..., 2])) > 3 and (st[..., 2] == 1).any()        # unnormalised N': halves and quarters of 1, 3, 7


def test_fma32_rounds_once():
    rng = np.random.default_rng(0)
    a, b, c = (rng.normal(0, 1, 4000).astype(np.float32) * np.float32(2.0) ** rng.integers(-6, 7, 4000).astype(np.float32) for _ in range(3))
    a[:5], b[:5] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)                   # a b = 1 + 2^-11 + 2^-24: a tie but for c
    c[:5] = np.float32([0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -30, -2.0 ** -30])
    got = ex.fma32(a, b, c)
    want = np.float32([float(rnd32(F(x) * F(y) + F(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
