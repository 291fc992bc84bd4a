"""CPU half of the opaque-vote tests: the case table of tests/opaque_vote_cases.py against the kernels' sources, every case observable
by the float64 checkers alone, and check_alpha raising on the outputs a wrong vote would produce.

Observability is worked out for the hardest odd texel a case uses -- alpha 0 (RGBA8 code 0); the float frames' odd alpha of -3 moves
the reference four times as far, the filters being linear in the colour they average.  The weights of a reference do not depend on
alpha, so one call of a checker carries up to four cases: the image it averages holds one case's alpha plane per channel.
"""
import contextlib
import functools
import os
import re

import numpy as np
import pytest
import torch

import f64_checker
import np_bilateral_joint
import np_bilateral_temporal as nbt
import np_nlm_layers
import np_nlm_layers_temporal as nlt
import opaque_vote_cases as ov
from conftest import ROOT

CSRC = os.path.join(ROOT, "image_denoising_filter_amd", "csrc")
CPU = torch.device("cpu")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@contextlib.contextmanager
def one_torch_thread():
    """A single frame's tensors are a few thousand texels: one thread is 2.5 x faster than the pool (the batched pair sums are not)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


# ---- the table against the sources ----------------------------------------------------------------------------------------------------
def test_bilateral_shapes_are_the_sources():
    src = _src("bilateral_shapes.hpp")
    found = {int(r): (int(p), int(nw)) for c, r, p, nw in re.findall(r"case\s+(\d+):\s*return tuned\(BilShape<(\d+),\s*(\d+),\s*(\d+)>\{\}\)", src)
             if c == r}
    assert found == ov.BIL_SHAPES
    assert len(re.findall(r"return tuned\(", src)) == len(ov.BIL_SHAPES), "a tuned radius the table does not know"
    for name in ("bilateral.hip", "bilateral_temporal.hip"):
        k = _src(name)
        assert re.search(r"constexpr int TILE_W = 64, TILE_H = NW \* P;", k), name
        assert re.search(r"constexpr int LW = TILE_W \+ 2 \* R, LH = TILE_H \+ 2 \* R;", k), name
        assert re.search(r"X0 - R, Y0 - R, tid, NW \* 64,[^;]*&mine\)", k), name


def test_joint_bilateral_shapes_are_the_sources():
    """bilateral_joint.hip takes its shapes from bilateral_shapes.hpp (no list of its own) and fills LW x LH from (X0 - R, Y0 - R) with
    NW * 64 threads in trips of four texels: the colour tile and layer 0 in one loop, with the vote flag and the held word, further
    layers into the planes behind."""
    k = _src("bilateral_joint.hip")
    assert '#include "bilateral_shapes.hpp"' in k and "BilShape<" not in k
    assert re.search(r"return bil_for_radius\(radius,\s*\[&\]\(auto sh\) \{ return launch_joint_tiled<decltype\(sh\)::R, decltype\(sh\)::P, decltype\(sh\)::NW>\(ctx, a, s\); \},", k)
    assert re.search(r"template <int R, int P, int NW, int MAXL>\s*__global__ __launch_bounds__\(NW \* 64\) void bilateral_joint_kernel\(", k)
    assert re.search(r"constexpr int TILE_W = 64, TILE_H = NW \* P;", k)
    assert re.search(r"constexpr int LW = TILE_W \+ 2 \* R, LH = TILE_H \+ 2 \* R, N = LW \* LH;", k)
    assert re.search(r"fill_colour_and_planes_any\(img_t, gde_t, LW, LH, nb_frame\(a, f\), a\.fmt, nb_layer\(a, f, 0\), a\.gfmt, w, h, X0 - R, Y0 - R, tid, NW \* 64,"
                     r"\s*a\.scl\[0\], &mine, &held\);", k)
    assert re.search(r"fill_planes_any\(gde_t \+ \(size_t\)3 \* l \* N, LW, LH, nb_layer\(a, f, l\), a\.gfmt, w, h, X0 - R, Y0 - R, tid, NW \* 64, a\.scl\[l\]\);", k)
    assert len(re.findall(r"for \(int t0 = tid; t0 < n; t0 \+= 4 \* nthreads\)", k)) == 2, "both fills: four texels per thread and trip"
    assert re.search(r"if \(held && t == 0\) \*held = v\[j\]\.x \* sc; else g\[t\] = v\[j\]\.x \* sc;", k), "slot 0 of layer 0's x plane carries the vote"
    assert int(re.search(r"constexpr int kJointTiledLayers = (\d+);", k).group(1)) == ov.JOINT_TILED_LAYERS
    assert re.search(r"constexpr int kBilRtP = (\d+), kBilRtNW = (\d+);", _src("bilateral_shapes.hpp")).groups() == tuple(str(x) for x in ov.BIL_RT_SHAPE)
    assert {R: tuple(L for L in range(1, 5) if ov.joint_class(R, L) == "tuned") for R in ov.BIL_SHAPES} == ov.JOINT_LAYERS


def test_nlm_layer_shapes_are_the_sources():
    """Both files keep their shape constants and their colour-tile fill; the tile's geometry is nlm_guide.hpp's GuideTile, which the
    kernels read by name and beside which they state no formula of their own."""
    g = _src("nlm_guide.hpp")
    assert re.search(r"static constexpr int SLO = SLO_, SHI = SHI_, PLO = PLO_, PHI = PHI_, R = R_, NW = NW_;", g)
    assert re.search(r"static constexpr int PW = PHI - PLO, [^;]*TILE_H = NW \* R;", g)
    assert re.search(r"static constexpr int SW = SHI - SLO, LW = 64 \+ SW - 1;", g)
    assert re.search(r"static constexpr int LHC = TILE_H \+ SW - 1;", g)
    for name, kern in (("nlm_layers.hip", "a.in"), ("nlm_layers_temporal.hip", "nb")):
        k = _src(name)
        m = re.search(r"constexpr int kLR = (\d+), kLNW = (\d+);", k)
        assert m and (int(m.group(1)), int(m.group(2))) == ov.NLM_LAYERS_SHAPE, name
        assert '#include "nlm_guide.hpp"' in k, name
        assert re.search(r"using T = GuideTile<SLO, SHI, PLO, PHI, kLR, kLNW>;", k), name
        assert re.search(r"constexpr int R = T::R, NW = T::NW, PW = T::PW, DR = T::DR, NL = T::NL, NR = T::NR, VW = T::VW, TILE_H = T::TILE_H;\s*"
                         r"constexpr int SW = T::SW, LW = T::LW, LHC = T::LHC, LHG = T::LHG;", k), name
        assert not re.search(r"constexpr int (LW|LHC|SW|TILE_H|NW) = [^T]", k), name
        assert re.search(r"fill_tile<MID_FMT_RGBA32F, false>\(ctile, LW, LHC, " + re.escape(kern) + r", w, h, X0 \+ PLO \+ SLO, Y0 \+ SLO, tid, NW \* 64, 1\.0f, &mine\)", k), name


def test_nlm_strip_shapes_are_the_sources():
    strip, small, nlm = _src("nlm_strip.hpp"), _src("nlm_small.hip"), _src("nlm.hip")
    assert re.search(r"const int LW = 64 \+ SW - 1;\s*const int LH = TILE_H \+ PW - 1 \+ SW - 1;", strip)
    assert re.search(r"fill_tile<FMT, false>\(lds, LW, LH, nb, w, h, X0 \+ PLO \+ slo, Y0 \+ PLO \+ slo, tid, NW \* 64, a\.sk, opaque\)", strip)
    assert int(re.search(r"constexpr unsigned kNlmSmallRounds = (\d+);", strip).group(1)) == ov.NLM_SMALL_ROUNDS
    assert re.search(r"cdiv\(\(unsigned\)w, \(unsigned\)\(64 - \(patch_w - 1\)\)\) \* cdiv\(\(unsigned\)h, 32u\) \* \(unsigned\)frames", strip)
    shapes = {(int(r), int(nw)) for r, nw in re.findall(r"launch_strip<SLO, SHI, PLO, PHI, (\d+), (\d+),", small)}
    assert shapes == set(ov.NLM_STRIP_SHAPES.values())
    assert re.search(r"return rem > 0 && rem <= cu_count;", small) and re.search(r"const unsigned slots = 2u \* \(unsigned\)ctx->cu_count;", small)
    tuned = {((int(a), int(b)), (int(c), int(d))) for a, b, c, d, r, nw in re.findall(r"launch_strip<(-?\d+), (-?\d+), (-?\d+), (-?\d+), (\d+), (\d+),", nlm)
             if (int(r), int(nw)) == ov.NLM_STRIP_SHAPES["whole"]}
    assert tuned == set(ov.NLM_WINDOWS.values())


def test_positions_lie_in_the_interior_tile_and_name_the_slots():
    assert ov.bil_tile(20)[1:6] == (-20, -20, 104, 48, 512) and ov.frame_size(ov.bil_tile(20)) == (53, 151)
    assert ov.nlm_strip_tile("bench")[1:6] == (-13, -13, 84, 58, 256) and ov.nlm_strip_tile("bench", "half").threads == 512
    assert ov.nlm_layers_tile("bench")[1:6] == (-13, -10, 84, 84, 512) and ov.nlm_layers_tile("ref")[1:6] == (-10, -7, 77, 77, 512)
    for R in ov.BIL_SHAPES:
        t = ov.bil_tile(R)
        _, _, X0, Y0 = ov.interior_tile(t)
        ps = {p.name: p for p in ov.positions(t)}
        assert ps["slot 0"].xy == (X0 - R, Y0 - R) and ps["slot n-1"].xy == (X0 + 63 + R, Y0 + t.out_h - 1 + R)
        assert not any(p.note for p in ps.values()), "a bilateral output reads every slot of its tile"
    for name, h_w, (a, b), pname, (x, y), note in ov.case_table():
        assert 0 <= x < h_w[1] and 0 <= y < h_w[0], (name, pname)
    for t in [ov.bil_tile(R) for R in ov.BIL_SHAPES] + [ov.nlm_strip_tile(w_, s) for w_ in ov.NLM_WINDOWS for s in ("whole", "half")] + \
             [ov.nlm_layers_tile(w_) for w_ in ov.NLM_WINDOWS]:
        a, b, X0, Y0 = ov.interior_tile(t)
        h, w = ov.frame_size(t)
        assert X0 + t.ox >= 0 and Y0 + t.oy >= 0 and X0 + t.ox + t.lw <= w and Y0 + t.oy + t.lh <= h, "the LDS tile is inside the frame"
        assert -(-w // t.out_w) >= 3 and a >= 1 and b >= 1
        rows, cols = ov.tile_outputs(t, a, b, h, w)
        for p in ov.positions(t):
            assert 0 <= p.slot < t.lw * t.lh and t.cols[0] <= p.slot % t.lw <= t.cols[1] and t.rows[0] <= p.slot // t.lw <= t.rows[1]
            # some output of the interior tile reads the texel's alpha
            assert ov.window_mask(h, w, [p.xy], t.reach)[rows, cols].any(), (t.name, p.name)
    # the dispatcher's arithmetic at 256 CUs: one small frame is all HALF, 57 of them whole strips + a HALF tail, 92 wider ones the long copy
    assert ov.frame_size(ov.nlm_strip_tile("bench")) == (87, 139)
    assert ov.nlm_launch_shape(139, 87, 7, 1, 256) == dict(copy="small", whole=0, half=9)
    assert ov.nlm_launch_shape(139, 87, 7, 57, 256) == dict(copy="small", whole=512, half=1)
    assert ov.nlm_launch_shape(754, 87, 7, 92, 256) == dict(copy="long", whole=3588, half=0)


# ---- every case is observable -----------------------------------------------------------------------------------------------------------
def _as_ref(alpha):
    out = np.zeros(alpha.shape + (4,))
    out[..., 3] = alpha
    return out


def _packed(h, w, group):
    A = np.ones((h, w, 4), np.float32)
    for c, p in enumerate(group):
        A[p.xy[1], p.xy[0], c] = 0.0
    return A


def _groups(ps):
    return [ps[i:i + 4] for i in range(0, len(ps), 4)]


@functools.lru_cache(None)
def bil_single(R, variant):
    """{position name: (xy, alpha [h, w], den [h, w])} of the float64 checker for the single-frame bilateral forms."""
    t = ov.bil_tile(R)
    h, w = ov.frame_size(t)
    frames, layers = ov.base_frames(t, np.uint8)
    frame, (g1, g2) = frames[0], layers[0]
    guides = {"texture": [frame], "linear": [frame], "accum": [g1], "fused": [g1, g2]}[variant]
    out = {}
    for group in _groups(ov.bil_positions(R, variant == "linear")):
        num = den = 0
        for g in guides:
            with one_torch_thread():
                n_, d_ = f64_checker.bilateral_sums(_packed(h, w, group), ov.decode(g), R, ov.sigma_s(R), ov.SIGMA_C, variant == "linear", CPU)
            num, den = num + n_.numpy(), den + d_.numpy()
        for c, p in enumerate(group):
            out[p.name] = (p.xy, num[..., c] / den, den)
    return out


@pytest.mark.parametrize("variant", ["texture", "linear", "accum", "fused"])
@pytest.mark.parametrize("R", list(ov.BIL_SHAPES))
def test_single_frame_bilateral_cases_are_observable(R, variant):
    t = ov.bil_tile(R)
    worst = min(ov.check_alpha(_as_ref(al), _as_ref(al), [xy], t.reach, ov.BIL_TOL, variant == "linear")[1] for xy, al, _ in bil_single(R, variant).values())
    print(f"bilateral r={R} {variant}: smallest window deviation {worst:.3g}")


@functools.lru_cache(None)
def bil_temporal(R, layered):
    """{(sequence index, position name): (xy, [alpha of output t])}: np_bilateral_temporal on frames whose channels are the alpha planes
    of the sequence's three positions (the plain form's guide, the frames' own rgb, goes in as a one-layer guide)."""
    t = ov.bil_tile(R)
    h, w = ov.frame_size(t)
    frames, layers = ov.base_frames(t, np.float32)
    guides = layers if layered else [[f] for f in frames]
    out = {}
    for i, (n, k, f_odd) in enumerate(ov.SEQUENCES):
        group = ov.seq_positions(t, i)
        packed = [_packed(h, w, group if f == f_odd else []) for f in range(n)]
        outs = nbt.bilateral_temporal(packed, k, R, ov.sigma_s(R), ov.SIGMA_C, layers=guides[:n], dev=CPU)
        for c, p in enumerate(group):
            out[(i, p.name)] = (p.xy, [o[..., c] for o in outs])
    return out


def _check_sequence(cases, sequences, tile, tol, exact_outside=True):
    worst = np.inf
    for (i, _), (xy, alphas) in cases.items():
        n, k, f_odd = sequences[i]
        for t_out, al in enumerate(alphas):
            if ov.placement(n, k, f_odd, t_out) == "unseen":
                if exact_outside:
                    assert np.all(al[ov.interior_mask(*al.shape, tile.reach)] == 1.0)
                continue
            worst = min(worst, ov.check_alpha(_as_ref(al), _as_ref(al), [xy], tile.reach, tol, exact_outside=exact_outside)[1])
    return worst


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("R", list(ov.BIL_SHAPES))
def test_bilateral_over_neighbouring_frames_cases_are_observable(R, layered):
    worst = _check_sequence(bil_temporal(R, layered), ov.SEQUENCES, ov.bil_tile(R), ov.BIL_TOL)
    print(f"bilateral over neighbouring frames r={R} {'2 layers' if layered else 'plain'}: smallest window deviation {worst:.3g}")


@functools.lru_cache(None)
def nlm_layers_single(window, n_layers):
    t = ov.nlm_layers_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    guides = ov.base_frames(t, np.float32)[1][0][:n_layers]
    out = {}
    for group in _groups(ov.positions(t)):
        num, den = np_nlm_layers.nlm_layers_sums(_packed(h, w, group), guides, ov.HPARAM, search, patch)
        for c, p in enumerate(group):
            out[p.name] = (p.xy, num[..., c] / den, den)
    return out


@functools.lru_cache(None)
def nlm_layers_temporal(window):
    t = ov.nlm_layers_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    _, layers = ov.base_frames(t, np.float32)
    ones = np.ones((h, w, 4), np.float32)
    sums = functools.lru_cache(None)(lambda t_, f, l: nlt.pair_sums(layers[t_][l], layers[f][l], ones, ov.HPARAM, search, patch))
    out = {}
    for i, (n, k, f_odd) in enumerate(ov.NLM_SEQUENCES[window]):
        group = ov.seq_positions(t, i)
        alphas = []
        for t_out in range(n):
            num, den = np.zeros((h, w, 4)), np.zeros((h, w))
            for f in range(max(0, t_out - k), min(n - 1, t_out + k) + 1):
                for l in range(2):
                    pn, pd = sums(t_out, f, l) if f != f_odd else nlt.pair_sums(layers[t_out][l], layers[f][l], _packed(h, w, group), ov.HPARAM, search, patch)
                    num, den = num + pn, den + pd
            alphas.append(num / den[..., None])
        for c, p in enumerate(group):
            out[(i, p.name)] = (p.xy, [a[..., c] for a in alphas])
    return out


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_layer_guided_nlm_cases_are_observable(window):
    t = ov.nlm_layers_tile(window)
    for n_layers in (1, 2):
        worst = min(ov.check_alpha(_as_ref(al), _as_ref(al), [xy], t.reach, ov.NLM_TOL, exact_outside=False)[1]
                    for xy, al, _ in nlm_layers_single(window, n_layers).values())
        print(f"layer-guided nlm {window} L={n_layers}: smallest window deviation {worst:.3g}")
    worst = _check_sequence(nlm_layers_temporal(window), ov.NLM_SEQUENCES[window], t, ov.NLM_TOL, exact_outside=False)
    print(f"layer-guided nlm over neighbouring frames {window} L=2: smallest window deviation {worst:.3g}")


@functools.lru_cache(None)
def nlm_single(window):
    t = ov.nlm_strip_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    frame = ov.base_frames(t, np.float32)[0][0]
    out = {}
    for p in ov.strip_positions(window):
        odd = ov.with_odd(frame, p.xy, 0.0)
        num, den = f64_checker.nlm_sums(odd, [odd], ov.HPARAM, search, patch, CPU)
        out[p.xy] = (p.xy, (num[..., 3] / den).numpy(), den.numpy())
    return out


@functools.lru_cache(None)
def nlm_temporal(window):
    t = ov.nlm_strip_tile(window)
    h, w = ov.frame_size(t)
    search, patch = ov.NLM_WINDOWS[window]
    frames, _ = ov.base_frames(t, np.float32)
    @functools.lru_cache(None)
    def base(t_, f):
        num, den = f64_checker.nlm_sums(frames[t_], [frames[f]], ov.HPARAM, search, patch, CPU)
        return num[..., 3].numpy(), den.numpy()
    out = {}
    for i, (n, k, f_odd) in enumerate(ov.NLM_SEQUENCES[window]):
        for p in ov.seq_positions(t, i):
            odd = ov.with_odd(frames[f_odd], p.xy, 0.0)
            alphas = []
            for t_out in range(n):
                win = range(max(0, t_out - k), min(n - 1, t_out + k) + 1)
                d = sum(base(t_out, f)[1] for f in win)
                a = sum(base(t_out, f)[0] for f in win if f != f_odd)
                if f_odd in win:
                    a = a + f64_checker.nlm_sums(frames[t_out], [odd], ov.HPARAM, search, patch, CPU)[0][..., 3].numpy()
                alphas.append(a / d)
            out[(i, p.name)] = (p.xy, alphas)
    return out


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_plain_nlm_cases_are_observable(window):
    t = ov.nlm_strip_tile(window)
    worst = min(ov.check_alpha(_as_ref(al), _as_ref(al), [xy], t.reach, ov.NLM_TOL, exact_outside=False)[1] for xy, al, _ in nlm_single(window).values())
    print(f"plain nlm {window} k=0: smallest window deviation {worst:.3g}")
    worst = _check_sequence(nlm_temporal(window), ov.NLM_SEQUENCES[window], t, ov.NLM_TOL, exact_outside=False)
    print(f"plain nlm over neighbouring frames {window}: smallest window deviation {worst:.3g}")


def test_a_float_frames_odd_alpha_moves_the_reference_four_times_as_far():
    t = ov.bil_tile(4)
    h, w = ov.frame_size(t)
    p = ov.positions(t)[0]
    frame = ov.flat_frame(np.random.default_rng(5), h, w, np.float32)
    dev = []
    for alpha in (0.0, ov.ODD_ALPHA[np.dtype(np.float32)]):
        odd = ov.with_odd(frame, p.xy, alpha)
        num, den = f64_checker.bilateral_sums(odd, odd, 4, ov.sigma_s(4), ov.SIGMA_C, False, CPU)
        dev.append(1.0 - (num[..., 3] / den).numpy()[ov.window_mask(h, w, [p.xy], t.reach)])
    assert np.allclose(dev[1], 4.0 * dev[0], rtol=1e-12, atol=0)


# ---- the check would catch the bug ------------------------------------------------------------------------------------------------------
def _tile_block(t, al):
    a, b, _, _ = ov.interior_tile(t)
    return ov.tile_outputs(t, a, b, *al.shape)


@pytest.mark.parametrize("slot", ["slot 0", "slot n-1"])
@pytest.mark.parametrize("R,variant", [(8, "texture"), (20, "linear"), (10, "fused")])
def test_check_alpha_raises_on_a_bilateral_tile_that_voted_opaque(R, variant, slot):
    """The one tile that sees the texel at `slot` writes alpha == 1.0 for all its outputs, every other tile is right."""
    t = ov.bil_tile(R)
    xy, al, _ = bil_single(R, variant)[slot]
    ref = _as_ref(al)
    ov.check_alpha(ref, ref, [xy], t.reach, ov.BIL_TOL, variant == "linear")
    bad = ref.copy()
    bad[_tile_block(t, al) + (3,)] = 1.0
    assert not np.array_equal(bad, ref)
    with pytest.raises(AssertionError, match="alpha off by"):
        ov.check_alpha(bad, ref, [xy], t.reach, ov.BIL_TOL, variant == "linear")


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
@pytest.mark.parametrize("slot", ["slot 0", "slot n-1"])
def test_check_alpha_raises_on_an_nlm_tile_that_voted_opaque(window, slot):
    """NLM's opaque form sets normWeight = 0.001 + sum(w * alpha): the tile's alpha becomes num / (0.001 + num) (and its rgb is
    divided by the same wrong norm)."""
    t = ov.nlm_strip_tile(window)
    p = next(q for q in ov.positions(t) if q.name == slot)
    xy, al, den = nlm_single(window)[p.xy]
    ref = _as_ref(al)
    blk = _tile_block(t, al)
    bad = ref.copy()
    num = (al * den)[blk]
    bad[blk + (3,)] = num / (0.001 + num)
    with pytest.raises(AssertionError, match="alpha off by"):
        ov.check_alpha(bad, ref, [xy], t.reach, ov.NLM_TOL, exact_outside=False)
    tl = ov.nlm_layers_tile(window)
    xy, al, den = nlm_layers_single(window, 2)[slot]
    ref, blk = _as_ref(al), _tile_block(tl, al)
    bad = ref.copy()
    num = (al * den)[blk]
    bad[blk + (3,)] = num / (2 * 0.001 + num)
    with pytest.raises(AssertionError, match="alpha off by"):
        ov.check_alpha(bad, ref, [xy], tl.reach, ov.NLM_TOL, exact_outside=False)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("R", [8, 20])
def test_check_alpha_raises_on_a_vote_left_over_from_the_previous_neighbour(R, layered):
    """Sequence (3, 2, 2): the odd frame is the LAST neighbour of every output.  A flag left over from the neighbour before it keeps the
    tile on the opaque form, which is the last neighbour's contribution computed with alpha forced to 1."""
    t = ov.bil_tile(R)
    i = ov.SEQUENCES.index((3, 2, 2))
    h, w = ov.frame_size(t)
    frames, layers = ov.base_frames(t, np.float32)                                     # bil_temporal's frames
    stale = nbt.bilateral_temporal([np.ones((h, w, 4), np.float32)] * 3, 2, R, ov.sigma_s(R), ov.SIGMA_C,
                                   layers=(layers if layered else [[f] for f in frames])[:3], dev=CPU)
    for slot in ("slot 0", "slot n-1"):
        xy, alphas = bil_temporal(R, layered)[(i, slot)]
        for t_out, al in enumerate(alphas):
            ref = _as_ref(al)
            bad = ref.copy()
            blk = _tile_block(t, al)
            bad[blk + (3,)] = stale[t_out][..., 3][blk]
            with pytest.raises(AssertionError, match="alpha off by"):
                ov.check_alpha(bad, ref, [xy], t.reach, ov.BIL_TOL)


def test_check_alpha_refuses_a_blind_case():
    """sigma_s = R / 2.5, the suite's usual choice: the far corner's tap weighs e^-6 of the centre's and the guard says so."""
    t = ov.bil_tile(8)
    h, w = ov.frame_size(t)
    p = ov.positions(t)[0]
    frame = ov.with_odd(ov.flat_frame(np.random.default_rng(6), h, w, np.float32), p.xy, 0.25)
    num, den = f64_checker.bilateral_sums(frame, frame, 8, 2.0, ov.SIGMA_C, False, CPU)
    ref = (num / den[..., None]).numpy()
    with pytest.raises(AssertionError, match="blind case"):
        ov.check_alpha(ref, ref, [p.xy], t.reach, ov.BIL_TOL)


# ---- the joint (cross) bilateral ------------------------------------------------------------------------------------------------------
# The references here are the ones tests/test_gpu_bilateral_joint_vote.py compares the kernels with (opaque_vote_cases.joint_refs, cached):
# RGBA8 frames carry the hardest odd texel, alpha 0; the float frames' -3 moves alpha four times as far, so their cases are checked a
# second time with the deviation divided by four, which is what an alpha-0 texel would give.
JOINT_CASES = [(R, L) for R in ov.JOINT_LAYERS for L in ov.JOINT_LAYERS[R]]


def _joint_seen(R, L):
    """(dtype, sequence, position, output t, placement, ref) of every comparison of a joint case in which the output sees the odd frame."""
    for (dt, i), (group, refs) in ov.joint_refs(R, L).items():
        n, k, f_odd = ov.SEQUENCES[i]
        for t_out in range(n):
            place = ov.placement(n, k, f_odd, t_out)
            for p in group:
                yield dt, i, p, t_out, place, refs[t_out][p.name]


@pytest.mark.parametrize("R,L", JOINT_CASES)
def test_joint_bilateral_cases_are_observable(R, L):
    t = ov.bil_tile(R)
    worst, placements = np.inf, set()
    for dt, i, p, t_out, place, ref in _joint_seen(R, L):
        if place == "unseen":
            assert np.all(np.abs(ref[..., 3][ov.interior_mask(*ref.shape[:2], t.reach)] - 1.0) <= 1e-12)
            continue
        placements.add(place)
        dev = ov.check_alpha(ref, ref, [p.xy], t.reach, ov.BIL_TOL)[1]
        if dt == np.float32:
            zero = ref.copy()
            zero[..., 3] = 1.0 - (1.0 - ref[..., 3]) / (1.0 - ov.odd_value(dt))
            dev = ov.check_alpha(zero, zero, [p.xy], t.reach, ov.BIL_TOL)[1]
        worst = min(worst, dev)
    assert placements == ({"first", "last", "target"} | ({"middle"} if R != 20 else set()))
    print(f"joint bilateral r={R} L={L}: smallest window deviation {worst:.3g} (odd alpha 0)")


def test_joint_reference_pairs_add_up_to_the_checkers_outputs():
    """joint_refs adds np_bilateral_joint.pair_sums per (output, neighbour); bilateral_joint is the reference: the same numbers, for
    the rgb of the frames as drawn and for a case's alpha, in a five-frame sequence at k = 2 and an RGBA8 one at k = 1."""
    R, L = 4, 4
    t = ov.bil_tile(R)
    layers = [ls[:L] for ls in ov.joint_layers(t)]
    for dt, i in ((np.dtype(np.float32), 2), (np.dtype(np.uint8), 0)):
        n, k, f_odd = ov.SEQUENCES[i]
        group, refs = ov.joint_refs(R, L)[(dt, i)]
        frames = ov.base_frames(t, dt)[0][:n]
        p = group[2]
        want = np_bilateral_joint.bilateral_joint([ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames)], layers[:n],
                                                  ov.JOINT_SIGMAS[:L], k, R, ov.sigma_s(R))
        for t_out in range(n):
            assert np.max(np.abs(refs[t_out][p.name] - want[t_out])) < 1e-13, (dt, t_out)
    assert len({id(ls[l]) for ls in layers for l in range(L)}) == 5 * L
    two = ov.base_frames(t, np.uint8)[1]
    assert all(np.array_equal(a, b) for ls, bs in zip(ov.joint_layers(t), two) for a, b in zip(ls, bs)), "layers 0 and 1 are base_frames' draws"


@pytest.mark.parametrize("R,L", JOINT_CASES)
def test_joint_bilateral_held_word_is_observable(R, L):
    """The odd texel at slot 0 is read by ONE output of the interior tile, (X0, Y0), through ONE tap, whose guide value in layer 0's x
    plane is the word the vote went through.  Were that word anything but the texel's value -- 0, or the vote's own 0 / 1 as bits --
    the tap's weight would change and with it the alpha of (X0, Y0): by at least 5 x tol, so that check_alpha's window comparison
    fails.  Worked out by the checker on the (2R+1)^2 window of that output alone, which is all the output reads."""
    t = ov.bil_tile(R)
    _, _, X0, Y0 = ov.interior_tile(t)
    crop = (slice(Y0 - R, Y0 + R + 1), slice(X0 - R, X0 + R + 1))
    layers = [[g[crop] for g in ls[:L]] for ls in ov.joint_layers(t)]
    smallest = np.inf
    for i in ov.JOINT_SEQUENCES[R]:
        n, k, f_odd = ov.SEQUENCES[i]
        p = ov.seq_positions(t, i)[0]
        assert p.name == "slot 0" and p.xy == (X0 - R, Y0 - R)
        alpha = [np.ones((2 * R + 1, 2 * R + 1, 4), np.float32) for _ in range(n)]
        alpha[f_odd][0, 0, :] = 0.0
        wrong = [[g.copy() for g in ls] for ls in layers[:n]]
        assert wrong[f_odd][0][0, 0, 0] >= 126
        wrong[f_odd][0][0, 0, 0] = 0
        args = (ov.JOINT_SIGMAS[:L], k, R, ov.sigma_s(R))
        drawn, zeroed = np_bilateral_joint.bilateral_joint(alpha, layers[:n], *args), np_bilateral_joint.bilateral_joint(alpha, wrong, *args)
        for t_out in range(n):
            if ov.placement(n, k, f_odd, t_out) in ("unseen", "target"):      # (the target's own centre comes from global memory, not from the tile)
                continue
            full = ov.joint_refs(R, L)[(np.dtype(np.float32), i)][1][t_out][p.name][Y0, X0, 3]
            assert abs((1.0 - drawn[t_out][R, R, 3]) * (1.0 - ov.odd_value(np.float32)) - (1.0 - full)) < 1e-12, "the window is the whole of what (X0, Y0) reads"
            smallest = min(smallest, abs(drawn[t_out][R, R, 3] - zeroed[t_out][R, R, 3]))
    assert smallest >= 5 * ov.BIL_TOL, f"a wrong held word moves alpha at (X0, Y0) by {smallest:.3g} only"
    print(f"joint bilateral r={R} L={L}: a zero in the held word moves alpha at (X0, Y0) by at least {smallest:.3g}")


@pytest.mark.parametrize("R,L", [(4, 4), (8, 2), (10, 1), (20, 1)])
def test_check_alpha_raises_on_a_joint_tile_that_voted_opaque(R, L):
    """The interior tile runs the opaque tap loop although its colour tile holds the odd texel: acc.w = accw for that neighbour, so
    every output of the tile has alpha exactly 1.0; every other tile is right."""
    t = ov.bil_tile(R)
    hit = 0
    for dt, i, p, t_out, place, ref in _joint_seen(R, L):
        if i != 0 or place == "unseen" or p.name not in ("slot 0", "slot n-1"):
            continue
        bad = ref.copy()
        bad[_tile_block(t, ref[..., 3]) + (3,)] = 1.0
        with pytest.raises(AssertionError, match="alpha off by"):
            ov.check_alpha(bad, ref, [p.xy], t.reach, ov.BIL_TOL)
        hit += 1
    assert hit == (12 if ov.JOINT_U8_SEQUENCES[R] else 6)


@pytest.mark.parametrize("R,L,seq", [(4, 4, (3, 2, 2)), (8, 2, (3, 2, 2)), (8, 4, (5, 2, 2)), (10, 1, (5, 2, 2))])
def test_check_alpha_raises_on_a_joint_vote_left_over_from_the_previous_neighbour(R, L, seq):
    """The odd frame follows an opaque neighbour in the window (placement 'last' or 'middle').  A vote kept from that neighbour runs the
    odd frame's taps in the opaque form: its alpha sum is its weight sum, and the tile's alpha, sum over the window of both, is 1.0."""
    t = ov.bil_tile(R)
    i = ov.SEQUENCES.index(seq)
    hit = 0
    for dt, j, p, t_out, place, ref in _joint_seen(R, L):
        if j != i or place not in ("last", "middle") or p.name not in ("slot 0", "slot n-1"):
            continue
        bad = ref.copy()
        bad[_tile_block(t, ref[..., 3]) + (3,)] = 1.0
        with pytest.raises(AssertionError, match="alpha off by"):
            ov.check_alpha(bad, ref, [p.xy], t.reach, ov.BIL_TOL)
        hit += 1
    assert hit == 2 * sum(ov.placement(*seq, t_out) in ("last", "middle") for t_out in range(seq[0]))
