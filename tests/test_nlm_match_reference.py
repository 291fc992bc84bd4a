"""tests/np_nlm_match.py -- the exact known answers tests/test_gpu_nlm_wide_windows.py holds the NLM kernels to at search windows up
to 64 wide -- on the CPU: the promises its frames rest on (power-of-two scales, palettes far enough apart that every weight is 0 or
1), agreement with the two float64 restatements of nonlocal.comp (tests/np_reference.py, tests/f64_checker.py) on small frames, and,
on the very frames of every GPU case, that a kernel off by one search row or column, or one patch row or column, would have failed
it: its alpha sums would differ at many pixels."""
import numpy as np
import pytest
import torch

import f64_checker
import np_nlm_match as npm
import np_reference as npr

CPU = torch.device("cpu")


def test_exact_h_gives_power_of_two_scales():
    sk, inv_sk, kexp = npm.kernel_scales(npm.EXACT_H)
    assert sk == np.float32(64.0) and inv_sk == np.float32(2.0 ** -6) and kexp == np.float32(-4096.0)


@pytest.mark.parametrize("palette,unit", [(npm.PALETTE_F, 1.0), (npm.PALETTE_U8, 1 / 255)])
def test_palettes_make_every_weight_zero_or_one(palette, unit):
    p = palette.astype(np.float64) * unit
    gap = np.abs(p[:, None, :] - p[None, :, :]).max(-1)
    np.fill_diagonal(gap, np.inf)
    nearest = min(gap.min(), np.abs(p).max(-1).min())       # to another entry, or to (0,0,0), the out-of-image texel
    assert nearest >= (0.5 if unit == 1.0 else 64 / 255) - 1e-12
    # one differing texel, scaled by sk = 64 as the strip kernels do (or d * kexp in the per-pixel kernel): below 2^-149
    assert -(nearest * 64.0) ** 2 < -150
    if unit == 1.0:
        # scaled colours with few mantissa bits: 4096 offsets of 1.5 * 64, and three frames of 4096 alpha codes <= 1023, stay exact
        assert np.array_equal(p * 64, np.round(p * 64)) and 4096 * 96 < 2 ** 24 and 3 * 4096 * 1023 < 2 ** 24


SMALL = [((-3, 4), (-1, 2)), ((-2, 3), (-2, 2)), ((-4, 2), (0, 1)), ((-3, 3), (-1, 3)), ((-5, 6), (-3, 4))]


@pytest.mark.parametrize("search,patch", SMALL)
def test_agrees_with_the_float64_restatements(search, patch):
    rng = np.random.default_rng(search[1] * 17 + patch[0])
    t = npm.pattern_frame(rng, 18, 23, search)
    nb = npm.with_defects(rng, t, 8)
    num, count = npm.match_sums(t, nb, search, patch)
    assert count.max() > 1
    assert np.array_equal(num[..., :3], count[..., None] * t[..., :3]), "a matching patch contains its centre"
    rn, rd = npr.nlm_sums(t, nb, npm.EXACT_H, search, patch)
    assert np.abs(rn - num).max() < 1e-9 and np.abs(rd - (0.001 + count)).max() < 1e-9
    cn, cd = f64_checker.nlm_sums(t, [nb], npm.EXACT_H, search, patch, dev=CPU)
    assert np.abs(cn.numpy() - num).max() < 1e-9 and np.abs(cd.numpy() - (0.001 + count)).max() < 1e-9
    # RGBA8: bytes compared, colours decoded as c / 255
    t8 = npm.pattern_frame(rng, 18, 23, search, npm.PALETTE_U8)
    nb8 = npm.with_defects(rng, t8, 8)
    num8, count8 = npm.match_sums(t8, nb8, search, patch)
    rn, rd = npr.nlm_sums(t8 / 255.0, nb8 / 255.0, npm.EXACT_H, search, patch)
    assert np.abs(rn - num8).max() < 1e-9 and np.abs(rd - (0.001 + count8)).max() < 1e-9


def test_temporal_sums_agree_with_the_float64_checker():
    search, patch = (-3, 4), (-1, 2)
    rng = np.random.default_rng(3)
    base = npm.pattern_frame(rng, 16, 21, search)
    frames = [npm.with_defects(rng, base, 5) for _ in range(4)]
    cache = {}
    for k in (0, 1, 2):
        for t in range(4):
            num, counts = npm.temporal_sums(frames, t, k, search, patch, cache)
            assert len(counts) == min(3, t + k) - max(0, t - k) + 1
            want = f64_checker.nlm_temporal_output(frames, t, k, npm.EXACT_H, search, patch, dev=CPU)
            got = num / (counts.sum(0) + 0.001 * len(counts))[..., None]
            assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()
            assert np.abs(npm.normalized_fp32(num, counts) - want).max() <= 4e-7 * np.abs(want).max()


def test_fp32_norm_is_the_kernels_sum():
    counts = np.array([[[0, 1, 700, 4095]], [[3, 0, 2048, 1]]])
    got = npm.fp32_norm(counts)
    for i in range(4):
        want = np.float32(0)
        for f in range(2):
            acc = np.float32(0.001)
            for _ in range(counts[f, 0, i]):
                acc = np.float32(acc + np.float32(1))
            want = np.float32(want + acc)
        assert got[0, i] == want
    assert np.all(np.abs(got - (counts.sum(0) + 0.002)) < 2e-3)


MANY = npm.CASE_SHAPE[0] * npm.CASE_SHAPE[1] // 100          # 1 % of the pixels of a case frame


@pytest.mark.parametrize("case", npm.WIDE_CASES, ids=npm.case_id)
def test_an_off_by_one_kernel_would_fail_the_gpu_case(case):
    """The alpha sums the GPU test asserts exactly, against those of a kernel that walks one search row or column too few, or
    takes the patch one row or column shorter (longer, for a 1x1 patch) at either end, or mirrored in one axis."""
    search, patch = case[:2]
    t, nb = npm.case_pair(case)
    base = npm.match_sums(t, nb, search, patch)[0][..., 3]
    for name, s, p in npm.off_by_one(search, patch):
        alt = npm.match_sums(t, nb, s, p)[0][..., 3]
        n = int((alt != base).sum())
        assert n >= MANY, (name, n)
