"""The strip kernels' fused distance-and-vertical-sum step (csrc/nlm_strip.hpp, planned by csrc/nlm_vbox_plan.hpp) on one ragged
frame, for a window of every fold class, against the float64 restatement tests/np_reference.py.

131 x 75: three tile columns, the last 15 wide (58-column tiles of the 7x7 patch), and three tile rows, the last holding one full
strip and a 3-row strip.  HDR noise; translucent texels in the top-left corner, so that the tiles there run the general loop form
and the others the opaque one.  A dropped or doubled distance row changes a patch distance by about 1/49 of itself and a weight by a
factor far outside the tolerance, so random data discriminates."""
import numpy as np
import pytest

import np_reference as npr
import oracle
from conftest import rel_err, synth_hdr

pytestmark = pytest.mark.gpu

NLM_TOL = 2e-5          # SURVEY.md 8c, as in test_gpu_parity.py
H, W = 75, 131
HP = 0.5
BENCH = dict(search=(-10, 11), patch=(-3, 4))

# window -> what the plan does with its distance rows (strips of eight rows unless noted)
WINDOWS = {
    "bench_7x7": BENCH,                                      # tuned: 12 of 14 rows fold
    "ref_6x6": dict(search=(-7, 7), patch=(-3, 3)),          # tuned: rows 0-4 fold, rows 7-11 feed two sums
    "rt_1x1": dict(search=(-2, 3), patch=(0, 1)),            # nothing folds: the additions stay where they were
    "rt_3x3": dict(search=(-2, 3), patch=(-1, 2)),           # 2 rows fold, 4 feed two sums
    "rt_6x6": dict(search=(-2, 3), patch=(-3, 3)),
    "rt_8x8": dict(search=(-2, 3), patch=(-4, 4)),           # 13 of 15
    "rt_9x9": dict(search=(-2, 3), patch=(-4, 5)),           # 14 of 16
    "rt_10x10": dict(search=(-2, 3), patch=(-5, 5)),         # strips of four rows
    "rt_16x16": dict(search=(-2, 3), patch=(-8, 8)),         # strips of four rows, the widest patch
}


def _tol(search):
    return NLM_TOL * max(1.0, (search[1] - search[0]) ** 2 / 441.0)     # (test_gpu_parity.py: test_nlm_unusual_windows)


@pytest.fixture(scope="module")
def frames():
    """Three float frames (the first one is the target of every test) and an RGBA8 pair."""
    rng = np.random.default_rng(20251)
    base = (synth_hdr(rng, H, W) * 0.25).astype(np.float32)
    fr = [(base * rng.gamma(16.0, 1 / 16.0, (H, W, 1))).astype(np.float32) for _ in range(3)]
    for f in fr:
        f[..., 3] = 1.0
        f[:20, :20, 3] = rng.uniform(0.25, 1.0, (20, 20)).astype(np.float32)
    u8 = [np.clip(f * 255.0 * 0.6, 0, 255).astype(np.uint8) for f in fr[:2]]
    for u in u8:
        u[..., 3] = 255
        u[:20, :20, 3] = rng.integers(64, 256, (20, 20), dtype=np.uint8)
    for a in fr + u8:
        a.setflags(write=False)
    return fr, u8


@pytest.fixture(scope="module")
def bench_sums(frames):
    """float64 sums of the first frame against itself and against the second, bench window: computed once, shared."""
    fr, _ = frames
    return [npr.nlm_sums(fr[0], nb, HP, **BENCH) for nb in fr[:2]]


def _normalized(num, den):
    return num / den[..., None]


@pytest.mark.parametrize("name", list(WINDOWS))
def test_window_against_float64(ctx, frames, bench_sums, name):
    fr, _ = frames
    cfg = WINDOWS[name]
    t = fr[0]
    num, den = bench_sums[0] if name == "bench_7x7" else npr.nlm_sums(t, t, HP, **cfg)
    fused = ctx.nlm_temporal([t], k=0, hparam=HP, **cfg)[0]
    Wg = ctx.nlm_accum(t, t, np.zeros((H, W, 8), np.float32), HP, **cfg)
    tol = _tol(cfg["search"])
    e_acc = max(rel_err(Wg[..., :4], num), rel_err(Wg[..., 4], den))
    e_fused = rel_err(fused, _normalized(num, den))
    print(f"{name}: accumulate {e_acc:.2e} fused {e_fused:.2e} (tolerance {tol:.1e})")
    assert e_acc < tol and e_fused < tol
    assert np.array_equal(fused, ctx.normalize(Wg)), "fused == accumulate + normalize, bit for bit"


def test_bench_window_neighbour_frame(ctx, frames, bench_sums):
    """target != neighbour (no zero distances at the centre offset), accumulate-only launch shape."""
    fr, _ = frames
    Wg = ctx.nlm_accum(fr[0], fr[1], np.zeros((H, W, 8), np.float32), HP, **BENCH)
    num, den = bench_sums[1]
    assert max(rel_err(Wg[..., :4], num), rel_err(Wg[..., 4], den)) < NLM_TOL


def test_bench_window_rgba8(ctx, frames):
    _, u8 = frames
    t, nb = oracle.unpack_u8(u8[0], 0), oracle.unpack_u8(u8[1], 0)
    num, den = npr.nlm_sums(t, nb, HP, **BENCH)
    Wg = ctx.nlm_accum(u8[0], u8[1], np.zeros((H, W, 8), np.float32), HP, **BENCH)
    assert max(rel_err(Wg[..., :4], num), rel_err(Wg[..., 4], den)) < NLM_TOL
    num0, den0 = npr.nlm_sums(t, t, HP, search=(-2, 3), patch=(-3, 4))      # (and the 7x7 patch through the run-time-window kernel)
    W0 = ctx.nlm_accum(u8[0], u8[0], np.zeros((H, W, 8), np.float32), HP, search=(-2, 3), patch=(-3, 4))
    assert max(rel_err(W0[..., :4], num0), rel_err(W0[..., 4], den0)) < NLM_TOL


def test_bench_window_temporal_k1(ctx, frames, bench_sums):
    """The temporal kernel (k = 1, three frames): the first output frame adds the sums of frames 0 and 1; every output frame equals
    the dispatch sequence over its neighbour frames, normalized, bit for bit."""
    fr, _ = frames
    out = ctx.nlm_temporal(fr, k=1, hparam=HP, **BENCH)
    num = sum(s[0] for s in bench_sums)
    den = sum(s[1] for s in bench_sums)
    assert rel_err(out[0], _normalized(num, den)) < NLM_TOL
    for t in range(3):
        Wg = np.zeros((H, W, 8), np.float32)
        for f in range(max(0, t - 1), min(2, t + 1) + 1):
            Wg = ctx.nlm_accum(fr[t], fr[f], Wg, HP, **BENCH)
        assert np.array_equal(out[t], ctx.normalize(Wg)), t
