"""No GPU: the contract of half / float guide layers (include/mi_denoise.h, section a3) restated in fp32 against the float64
checker, and the Python layer's dtype rules.

The kernels carry a guide value as the fp32 product g * sqrt(0.5 log2 e) / colorSigma, so the precision of a weight falls off
as about 2^-24 |g| / colorSigma.  The GPU tests hold the kernels to the bilateral tolerance 1e-5 max(1, |ref|) on the inputs of
guide_format_inputs.py (max |g| <= 16 colorSigma); this file asserts that the CONTRACT ALONE -- fp32 arithmetic in the stated
order of magnitude, nothing of the kernels' code -- stays under HALF that tolerance on those same inputs, so the bound the GPU
tests assert comes from the number format and leaves the kernels the other half.
"""
import numpy as np
import pytest

import guide_format_inputs as gi
import np_bilateral_temporal as chk
from conftest import rel_err

SHAPE, R = (45, 133), 8


def test_inputs_meet_the_stated_condition():
    for dt in (np.float32, np.float16):
        ratio = gi.max_guide_ratio(gi.render_layers(SHAPE, 3, dt))
        print(f"{np.dtype(dt).name} guides: max |g| / sigma_c = {ratio:.2f}")
        assert 15.0 < ratio <= 16.0                 # inside the condition, and near its edge: the depth layer


@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
def test_fp32_restatement_stays_under_half_the_tolerance(dt):
    frames, layers = gi.hdr_frames(SHAPE, 2), gi.render_layers(SHAPE, 2, dt)
    worst = 0.0
    for l in range(3):                              # normals, albedo, depth: target frame 0, neighbour frame 1
        num, den = gi.fp32_pair_sums(layers[0][l], layers[1][l], frames[1], R, gi.SIGMA_S, gi.SIGMA_C)
        n64, d64 = chk.pair_sums(layers[0][l], layers[1][l], frames[1], R, gi.SIGMA_S, gi.SIGMA_C, dev="cpu")
        e = rel_err(num / den[..., None], chk.normalize(n64, d64))
        print(f"{np.dtype(dt).name} layer {l} ({('normals', 'albedo', 'depth')[l]}): fp32 contract against float64, worst rel err {e:.3e}")
        worst = max(worst, e)
    assert worst < 0.5 * gi.TOL


def test_python_dtype_rules():
    """The checks api.py makes before it touches the library: no GPU, no context."""
    from image_denoising_filter_amd import api
    h, w = 4, 8
    u8, f16, f32 = (np.zeros((h, w, 4), d) for d in (np.uint8, np.float16, np.float32))
    assert api._guide_fmt(api.FMT_RGBA32F, [u8, u8], "t") == api.FMT_RGBA32F                    # RGBA8 guides: the word of old
    assert api._guide_fmt(api.FMT_RGBA8, [], "t") == api.FMT_RGBA8
    assert api._guide_fmt(api.FMT_RGBA8, [f32], "t") == api.FMT_RGBA8 | ((api.FMT_RGBA32F + 1) << 8) == 0x101
    assert api._guide_fmt(api.FMT_RGBA16F, [f16, f16], "t") == api.FMT_RGBA16F | ((api.FMT_RGBA16F + 1) << 8) == 0x302
    assert api.fmt_with_guide(api.FMT_RGBA32F, api.FMT_RGBA8) == 0x200
    with pytest.raises(ValueError):
        api._guide_fmt(api.FMT_RGBA32F, [u8, f32], "t")                                         # one dtype per call
    with pytest.raises(TypeError):
        api._guide_fmt(api.FMT_RGBA32F, [np.zeros((h, w, 4), np.float64)], "t")
    both = (np.uint8, np.float16, np.float32)
    assert api._flat_layers([[f32, f32]], 1, h, w, "t", both)[0] == 2
    assert api._flat_layers([[f16], [f16]], 2, h, w, "t", both)[0] == 1
    with pytest.raises(ValueError):
        api._flat_layers([[f32], [f16]], 2, h, w, "t", both)                                    # mixed across frames
    with pytest.raises(ValueError):
        api._flat_layers([[u8, f32]], 1, h, w, "t", both)                                       # mixed inside a frame
    with pytest.raises(ValueError):
        api._flat_layers([[np.zeros((h, w, 4), np.float64)]], 1, h, w, "t", both)
    for bad in (f32, f16):                          # the NLM callers pass no dtypes: uint8 alone, as before
        with pytest.raises(ValueError):
            api._flat_layers([[bad]], 1, h, w, "nlm_layers_temporal")
    assert api._flat_layers([[u8]], 1, h, w, "nlm_layers_temporal")[0] == 1
