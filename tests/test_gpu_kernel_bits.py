"""Recorded output bits of the bilateral and layer-guided NLM kernels, single-frame and over neighbouring frames.

The kernels over neighbouring frames restate the tap / offset loops of the single-frame kernels (sharing the text cost speed on the
bench paths, LABNOTES R10.1), and the suite pins "temporal with k = 0 == single frame" bit for bit.  That identity notices a change
made to one copy; it cannot notice the same change made to both.  This file pins the bits themselves.
tests/golden/kernel_bits.json holds the sha256 of every case's output bytes, recorded from a known-good library (the bilateral
bench kernel's code hash of that library is stored beside them):

    MID_LIB_PATH=<that library> python tests/test_gpu_kernel_bits.py --record

and the tests assert the same hashes from the tree's library.  Inputs are closed-form integer patterns of x, y, channel, frame
and layer -- no RNG, so the fixture depends on no NumPy version.  Every case has an opaque variant and a translucent one (alpha
!= 1 for some texels with x < 40; tile columns further right stay fully opaque).

Shapes: the smallest that reach every path.  Bilateral 45 x 133: a partial tile row at 16- and 32-row tiles, two full tile columns
and a partial one; radii 4, 8, 10, 20 (tuned), 5 (run-time radius), 18 with layers (per pixel).  Layer-guided NLM 70 x 130: two
tile rows, one partial, three tile columns.  At these sizes only r = 4 / 5 has a tile whose halo stays inside the frame, and the
opaque form of the tap / offset loops needs such a tile, so a second shape per filter (74 x 148, 140 x 130) gives the larger
radii and the NLM windows one.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_bits.json")
NLM_CFGS = {"ref": dict(search=(-7, 7), patch=(-3, 3)), "bench": dict(search=(-10, 11), patch=(-3, 4)),
            "naive": dict(search=(-2, 3), patch=(-1, 3))}
BIL, BIL_IN = (45, 133), (74, 148)          # (h, w)
NLM, NLM_IN = (70, 130), (140, 130)
SS, SC, HP = 2.0, 0.2, 0.5


def frame(shape, f, translucent, dtype=np.float32):
    """Colours q / 64 with q = (x (3 + c) + y (5 + 2c) + 31 f + 17 c) mod 61: exact in fp16; RGBA8 frames hold 4 q."""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    q = np.stack([(x * (3 + c) + y * (5 + 2 * c) + 31 * f + 17 * c) % 61 for c in range(3)], -1)
    a = np.full((h, w), 64)
    if translucent:
        a = np.where((x < 40) & ((x + 2 * y + f) % 3 == 0), 16 * ((x + y) % 4), a)
    if dtype == np.uint8:
        return np.concatenate([q * 4, np.minimum(a * 4, 255)[..., None]], -1).astype(np.uint8)
    return (np.concatenate([q, a[..., None]], -1) / 64.0).astype(dtype)


def guide(shape, f, l):
    """An RGBA8 guide layer: ramps that wrap at 256, so neighbouring patches are close and some are not."""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    g = [(x * (2 + l) + 3 * y + 13 * f + 50 * l + 40 * c + (x * y) % 5) % 256 for c in range(3)]
    return np.stack(g + [np.full_like(x, 255)], -1).astype(np.uint8)


def cases():
    """{case id: function(ctx) -> list of arrays}.  Three frames and two layers per frame wherever a case needs them."""
    out = {}

    def add(name, fn):
        for tr in (False, True):
            out[f"{name}-{'translucent' if tr else 'opaque'}"] = (lambda ctx, fn=fn, tr=tr: fn(ctx, tr))

    def bilateral(shape, r, tag, fmt=np.float32):
        fr = lambda tr, n=3: [frame(shape, f, tr, fmt) for f in range(n)]
        gl = [[guide(shape, f, l) for l in range(2)] for f in range(3)]
        Z = np.zeros(shape + (8,), np.float32)
        if r != 18:                               # (the plain form's one tile fits LDS at every radius: per pixel only with layers)
            add(f"bil-{tag}-r{r}-texture", lambda c, tr: [c.bilateral(fr(tr)[0], r, SS, SC, "texture")])
            add(f"bil-{tag}-r{r}-linear", lambda c, tr: [c.bilateral(fr(tr)[0], r, SS, SC, "linear")])
            add(f"bil-{tag}-r{r}-batch2", lambda c, tr: c.bilateral_batch(fr(tr, 2), r, SS, SC, "texture"))
            add(f"bil-{tag}-r{r}-pair", lambda c, tr: [c.bilateral_pair_accum(fr(tr)[0], fr(tr)[1], Z, r, SS, SC)])
            add(f"bil-{tag}-r{r}-temporal", lambda c, tr: c.bilateral_temporal(fr(tr), 1, radius=r, sigma_s=SS, sigma_c=SC))
        add(f"bil-{tag}-r{r}-layers-accum", lambda c, tr: [c.bilateral_layers_accum(fr(tr)[0], gl[0][0], Z, r, SS, SC)])
        add(f"bil-{tag}-r{r}-layers-fused", lambda c, tr: [c.bilateral_layers(fr(tr)[0], gl[0], r, SS, SC)])
        add(f"bil-{tag}-r{r}-layers-pair", lambda c, tr: [c.bilateral_layers_pair_accum(gl[0][0], gl[1][0], fr(tr)[1], Z, r, SS, SC)])
        add(f"bil-{tag}-r{r}-layers-temporal", lambda c, tr: c.bilateral_temporal(fr(tr), 1, radius=r, sigma_s=SS, sigma_c=SC, layers=gl))

    for r in (4, 8, 10, 20, 5, 18):
        bilateral(BIL, r, "edge")
    for r in (8, 10, 20):
        bilateral(BIL_IN, r, "interior")
    # input formats and packed outputs, r = 8 only
    gl = [[guide(BIL, f, l) for l in range(2)] for f in range(3)]
    for name, dt in (("u8", np.uint8), ("f16", np.float16)):
        fr = lambda tr, dt=dt: [frame(BIL, f, tr, dt) for f in range(3)]
        add(f"bil-in-{name}-r8-texture", lambda c, tr, fr=fr: [c.bilateral(fr(tr)[0], 8, SS, SC, "texture")])
        add(f"bil-in-{name}-r8-linear", lambda c, tr, fr=fr: [c.bilateral(fr(tr)[0], 8, SS, SC, "linear")])
        add(f"bil-in-{name}-r8-layers-fused", lambda c, tr, fr=fr: [c.bilateral_layers(fr(tr)[0], gl[0], 8, SS, SC)])
        add(f"bil-in-{name}-r8-temporal", lambda c, tr, fr=fr: c.bilateral_temporal(fr(tr), 1, radius=8, sigma_s=SS, sigma_c=SC))
        f32 = lambda tr: [frame(BIL, f, tr) for f in range(3)]
        add(f"bil-out-{name}-r8-temporal", lambda c, tr, dt=dt: c.bilateral_temporal(f32(tr), 1, radius=8, sigma_s=SS, sigma_c=SC, out_dtype=dt))
        add(f"bil-out-{name}-r8-layers-temporal",
            lambda c, tr, dt=dt: c.bilateral_temporal(f32(tr), 1, radius=8, sigma_s=SS, sigma_c=SC, layers=gl, out_dtype=dt))
        add(f"bil-out-{name}-r8-sequence", lambda c, tr, dt=dt: c.sequence_bilateral(f32(tr)[:2], 8, SS, SC, out_dtype=dt)[0])
        add(f"bil-out-{name}-r8-layers-sequence", lambda c, tr, dt=dt: c.sequence_bilateral(f32(tr)[:2], 8, SS, SC, layers=gl[:2], out_dtype=dt)[0])

    def nlm(shape, cfg, tag):
        win = NLM_CFGS[cfg]
        fr = lambda tr, dt=np.float32: [frame(shape, f, tr, dt) for f in range(3)]
        gl = [[guide(shape, f, l) for l in range(2)] for f in range(3)]
        Z = np.zeros(shape + (8,), np.float32)
        add(f"nlm-{tag}-{cfg}-accum", lambda c, tr: [c.nlm_layers_accum(fr(tr)[0], gl[0][0], Z, HP, **win)])
        add(f"nlm-{tag}-{cfg}-fused", lambda c, tr: [c.nlm_layers(fr(tr)[0], gl[0], HP, **win)])
        add(f"nlm-{tag}-{cfg}-pair", lambda c, tr: [c.nlm_layers_pair_accum(gl[0][0], gl[1][0], fr(tr)[1], Z, HP, **win)])
        add(f"nlm-{tag}-{cfg}-temporal", lambda c, tr: c.nlm_layers_temporal(fr(tr), gl, 1, hparam=HP, **win))
        if tag == "edge" and cfg == "bench":      # packed input and output, once each
            add("nlm-in-u8-bench-temporal", lambda c, tr: c.nlm_layers_temporal(fr(tr, np.uint8), gl, 1, hparam=HP, **win))
            add("nlm-in-u8-bench-fused", lambda c, tr: [c.nlm_layers(fr(tr, np.uint8)[0], gl[0], HP, **win)])
            add("nlm-out-u8-bench-temporal", lambda c, tr: c.nlm_layers_temporal(fr(tr), gl, 1, hparam=HP, out_dtype=np.uint8, **win))
            add("nlm-out-u8-bench-sequence", lambda c, tr: c.sequence_nlm_layers(fr(tr)[:2], gl[:2], hparam=HP, out_dtype=np.uint8, **win)[0])

    for cfg in NLM_CFGS:
        nlm(NLM, cfg, "edge")
    for cfg in ("ref", "bench"):
        nlm(NLM_IN, cfg, "interior")
    return out


CASES = cases()


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["sha256"]


def test_every_case_is_recorded():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_output_bits(ctx, case):
    got = digest(CASES[case](ctx))
    assert got == recorded()[case], f"{case}: the output bytes are not the recorded ones"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(HERE))
    import image_denoising_filter_amd as mid
    from image_denoising_filter_amd import _codeobj
    with mid.Context(0) as c:
        sha = {name: digest(fn(c)) for name, fn in CASES.items()}
    with open(FIXTURE, "w") as f:
        json.dump({"recorded_from": {"bilateral_bench_kernel_sha256": _codeobj.fingerprint(mid.LIB_PATH, "bilateral")["kernel_code_sha256"]},
                   "sha256": sha}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(sha)} cases from {mid.LIB_PATH}")
