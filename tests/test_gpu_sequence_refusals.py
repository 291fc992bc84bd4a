"""The refusals every sequence entry point shares, pinned by text: (return code, mid_last_error()) of one call per broken rule
against tests/golden/sequence_refusals.json, which this module recorded from the library before the entry points' checks
became one function (csrc/pipeline.cpp, check_sequence):

    MID_LIB_PATH=<that library> python tests/test_gpu_sequence_refusals.py --record tests/golden/sequence_refusals.json

Every call of the refusal test starts from one valid call (3 frames of 8 x 16 texels, 2 guide layers each where the entry reads
layers, window k = 1, all three outputs) and breaks exactly one rule, so that test queues nothing and launches no kernel.  The three
mid_sequence_nlm_range* entries make no alias check (an output may be a frame there: every frame is uploaded before the first
output that could overwrite it), so the alias cases exist for the other five.  That those three still ACCEPT such an output, with
the bits of a call whose outputs are buffers of their own, is the module's second test, the only one here that runs kernels (three
8 x 16 frames per output format).  One entry of the table was edited by hand: mid_sequence_bilateral now words its "format names a
guide-layer format" refusal as bilateral_check_params does.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "sequence_refusals.json")
W, H, N, L, K = 8, 16, 3, 2, 1

# entry -> (parameter struct, has a layer table, has (k, first, count), has out_format, has layer_sigma, refuses aliased outputs)
ENTRIES = {
    "mid_sequence_nlm_range":           ("nlm", False, True, False, False, False),
    "mid_sequence_nlm_range_u8":        ("nlm", False, True, False, False, False),
    "mid_sequence_nlm_range_f16":       ("nlm", False, True, False, False, False),
    "mid_sequence_bilateral":           ("bil", True, False, True, False, True),
    "mid_sequence_nlm_layers":          ("nlm", True, False, True, False, True),
    "mid_sequence_nlm_layers_temporal": ("nlm", True, True, True, False, True),
    "mid_sequence_bilateral_temporal":  ("bil", True, True, True, False, True),
    "mid_sequence_bilateral_joint":     ("bil", True, True, True, True, True),
}


def _table(ptrs):
    return None if ptrs is None else (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def refusals(handle):
    """{"entry/case": [return code, message]} of every call of the module."""
    import image_denoising_filter_amd as mid
    from image_denoising_filter_amd._lib import BilateralParams, NlmParams, lib
    from image_denoising_filter_amd.api import fmt_with_guide

    # (host buffers the calls would read and write if one were accepted; 16 B per texel serves every format)
    bufs = [np.zeros((H, W, 4), np.float32) for _ in range(2 * N + N * 17)]
    frames = [b.ctypes.data for b in bufs[:N]]
    outs = [b.ctypes.data for b in bufs[N:2 * N]]
    layers17 = [b.ctypes.data for b in bufs[2 * N:]]
    layers = layers17[:N * L]
    got = {}
    for name, (params, layered, windowed, has_fmt, has_sigma, refuses_alias) in ENTRIES.items():
        def call(frames=frames, n=N, layers=layers, n_layers=L, k=K, first=0, count=N, outs=outs, out_fmt=mid.FMT_RGBA32F,
                 fmt=mid.FMT_RGBA32F):
            prm = NlmParams(W, H, 0.5, -2, 3, -1, 2, fmt) if params == "nlm" else \
                BilateralParams(W, H, 2.0, 0.2, 4, mid.LAYOUT_TEXTURE, fmt)
            args = [handle, ctypes.byref(prm)]
            if has_sigma:
                args.append(None)
            args += [_table(frames), n]
            if layered:
                args += [_table(layers), n_layers]
            if windowed:
                args += [k, first, count]
            args.append(_table(outs))
            if has_fmt:
                args.append(out_fmt)
            rc = getattr(lib, name)(*args, 1, None)
            return [rc, lib.mid_last_error().decode("utf-8", "replace") if rc else ""]

        def but(seq, i, value):
            return seq[:i] + [value] + seq[i + 1:]

        cases = {
            "frame table NULL": dict(frames=None),
            "output table NULL": dict(outs=None),
            "n_frames 0": dict(frames=[], n=0, layers=[], outs=[], count=0) if not windowed else dict(n=0),
            "a frame NULL": dict(frames=but(frames, 1, None)),
            "an output NULL": dict(outs=but(outs, 1, None)),
        }
        if windowed:
            cases.update({"k -1": dict(k=-1), "k beyond the ring": dict(k=48), "first -1": dict(first=-1), "count 0": dict(count=0),
                          "first + count > n": dict(first=1, count=N)})
        if has_fmt:
            cases["unknown output format"] = dict(out_fmt=99)
        if layered:
            cases["a layer NULL"] = dict(layers=but(layers, 3, None))
            cases["n_layers 17"] = dict(layers=layers17, n_layers=17)
        if refuses_alias:
            cases["an output is a frame"] = dict(outs=but(outs, 0, frames[1]))
            cases["an output twice"] = dict(outs=but(outs, 1, outs[0]))
            if layered:
                cases["an output is a layer"] = dict(outs=but(outs, 2, layers[1]))
        if name == "mid_sequence_bilateral":
            cases["guide-layer format without layers"] = dict(layers=None, n_layers=0,
                                                              fmt=fmt_with_guide(mid.FMT_RGBA32F, mid.FMT_RGBA16F))
        for case, change in cases.items():
            got[f"{name}/{case}"] = call(**change)
    return got


@pytest.mark.gpu
def test_gpu_sequence_refusals_match_the_recorded_table(ctx):
    with open(TABLE) as f:
        want = json.load(f)
    got = refusals(ctx.handle)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key][0] == 1 and got[key] == want[key], (key, got[key], want[key])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.float16])
def test_gpu_sequence_nlm_accepts_outputs_that_are_its_frames(ctx, dtype):
    """mid_sequence_nlm_range / _u8 / _f16 with out[t] = frame t: accepted, and the bits of the call with separate outputs."""
    import image_denoising_filter_amd as mid

    rng = np.random.default_rng(7)
    frames = [(rng.random((H, W, 4)) * 255).astype(dtype) if dtype == np.uint8 else rng.random((H, W, 4)).astype(dtype) for _ in range(N)]
    nlm = dict(k=K, hparam=0.5, search=(-2, 3), patch=(-1, 2))
    want, _ = ctx.sequence_nlm(frames, pinned=False, pinned_out=False, out_dtype=dtype, **nlm)
    bufs = [f.copy() for f in frames]
    ptrs = [b.ctypes.data for b in bufs]
    ctx.sequence_nlm_pinned(ptrs, ptrs, W, H, mid.api._fmt_of(frames[0]), out_dtype=dtype, **nlm)
    for got, ref, src in zip(bufs, want, frames):
        assert got.tobytes() == ref.tobytes() and got.tobytes() != src.tobytes()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import image_denoising_filter_amd as mid

    assert sys.argv[1] == "--record", __doc__
    with mid.Context(0) as c, open(sys.argv[2], "w") as f:
        json.dump(refusals(c.handle), f, indent=1, sort_keys=True)
        f.write("\n")
