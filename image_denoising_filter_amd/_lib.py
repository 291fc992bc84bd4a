"""ctypes loader for libmi_denoise.so (the C-ABI of include/mi_denoise.h).

The product path has no fallback: if the shared library is missing or does not load,
import of this module raises.  torch is imported FIRST on purpose: the PyTorch-ROCm wheel
carries its own libamdhip64.so.7, and a process must not end up with two HIP runtimes
(device pointers and streams would not be shared).  Loading torch first makes the
dynamic linker resolve this library's libamdhip64.so.7 dependency to the copy that is
already mapped, so torch tensors' data_ptr() and torch streams can be handed to the C-ABI.
"""
import ctypes
import os

import torch  # noqa: F401  (see module docstring: must precede the CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
# MID_LIB_PATH: development override used for A/B builds of the same C-ABI (never a fallback)
LIB_PATH = os.environ.get("MID_LIB_PATH") or os.path.join(_HERE, "libmi_denoise.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()). "
        "image_denoising_filter_amd has no CPU or PyTorch fallback."
    )

lib = ctypes.CDLL(LIB_PATH)

c_void_pp = ctypes.POINTER(ctypes.c_void_p)


class BilateralParams(ctypes.Structure):
    """mid_bilateral_params (first 16 bytes = the push-constant block of bialteral.comp:13-20)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("spatialSigma", ctypes.c_float), ("colorSigma", ctypes.c_float),
                ("radius", ctypes.c_int32), ("layout", ctypes.c_int32), ("format", ctypes.c_int32)]


class NlmParams(ctypes.Structure):
    """mid_nlm_params (first 12 bytes = the push-constant block of nonlocal.comp:16-22)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("filteringParameter", ctypes.c_float),
                ("search_lo", ctypes.c_int32), ("search_hi", ctypes.c_int32),
                ("patch_lo", ctypes.c_int32), ("patch_hi", ctypes.c_int32),
                ("format", ctypes.c_int32)]


class AtrousParams(ctypes.Structure):
    """mid_atrous_params (section a4g)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("first_pass", ctypes.c_int32), ("n_passes", ctypes.c_int32),
                ("colorSigma", ctypes.c_float), ("format", ctypes.c_int32)]


class AtrousMomentsParams(ctypes.Structure):
    """mid_atrous_moments_params (section a4i)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32)]


class AtrousVarianceParams(ctypes.Structure):
    """mid_atrous_variance_params (section a4i)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("first_pass", ctypes.c_int32), ("n_passes", ctypes.c_int32),
                ("sigmaLum", ctypes.c_float), ("epsilon", ctypes.c_float), ("format", ctypes.c_int32)]


class TemporalAccumParams(ctypes.Structure):
    """mid_temporal_accum_params (section a4j)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("alpha", ctypes.c_float), ("alphaMoments", ctypes.c_float),
                ("historyMax", ctypes.c_float), ("historyFull", ctypes.c_float), ("format", ctypes.c_int32)]


class AlbedoParams(ctypes.Structure):
    """mid_albedo_params (section a4k)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("floor", ctypes.c_float), ("format", ctypes.c_int32)]


class FireflyParams(ctypes.Structure):
    """mid_firefly_params (section a4l)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("radius", ctypes.c_int32), ("rank", ctypes.c_int32),
                ("gain", ctypes.c_float), ("floor", ctypes.c_float), ("format", ctypes.c_int32)]


class ColorBoundsParams(ctypes.Structure):
    """mid_color_bounds_params (section a4m)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("radius", ctypes.c_int32), ("gamma", ctypes.c_float),
                ("format", ctypes.c_int32)]


class ImageMetricsParams(ctypes.Structure):
    """mid_image_metrics_params (section a4n)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format_a", ctypes.c_int32), ("format_b", ctypes.c_int32),
                ("peak", ctypes.c_float), ("eps", ctypes.c_float), ("ssim", ctypes.c_int32)]


class ImageMetricsResult(ctypes.Structure):
    """mid_image_metrics_result (section a4n)."""
    _fields_ = [(name, ctypes.c_double) for name in ("n_valid", "n_invalid", "mse", "mse_r", "mse_g", "mse_b", "mae", "max_abs", "psnr",
                                                      "relmse", "ssim")]


METRICS_N = 16      # MID_METRICS_N


class GuidedParams(ctypes.Structure):
    """mid_guided_params (section a4o)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("radius", ctypes.c_int32), ("eps", ctypes.c_float),
                ("format", ctypes.c_int32)]


class MedianParams(ctypes.Structure):
    """mid_median_params (section a4p)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("radius", ctypes.c_int32), ("format", ctypes.c_int32)]


class NormalizeParams(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class Image(ctypes.Structure):
    """mid_image"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("format", ctypes.c_int32),
                ("data", ctypes.c_void_p)]


# every symbol include/mi_denoise.h declares, with its signature
_P = ctypes.c_void_p
_SIGNATURES = {
    "mid_ctx_create": (ctypes.c_int, [ctypes.c_int, c_void_pp]),
    "mid_ctx_destroy": (None, [_P]),
    "mid_ctx_release_cached": (ctypes.c_int, [_P]),
    "mid_last_error": (ctypes.c_char_p, []),
    "mid_version": (ctypes.c_int, []),
    "mid_ctx_stream_priorities": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_device_name": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_size_t]),
    "mid_alloc": (ctypes.c_int, [_P, ctypes.c_size_t, c_void_pp]),
    "mid_free": (ctypes.c_int, [_P, _P]),
    "mid_alloc_host": (ctypes.c_int, [_P, ctypes.c_size_t, c_void_pp]),
    "mid_free_host": (ctypes.c_int, [_P, _P]),
    "mid_host_register": (ctypes.c_int, [_P, _P, ctypes.c_size_t]),
    "mid_host_unregister": (ctypes.c_int, [_P, _P]),
    "mid_memcpy_h2d": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P]),
    "mid_memcpy_d2h": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P]),
    "mid_memset": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_size_t, _P]),
    "mid_stream_sync": (ctypes.c_int, [_P, _P]),
    "mid_bilateral": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), _P, _P, _P]),
    "mid_bilateral_batch": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), c_void_pp, c_void_pp, ctypes.c_int, _P]),
    "mid_bilateral_layers_accum": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), _P, _P, _P, _P]),
    "mid_bilateral_layers": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), _P, c_void_pp, ctypes.c_int, _P, _P]),
    "mid_nlm_accum": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), _P, _P, _P, _P]),
    "mid_nlm_temporal": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int, c_void_pp, _P]),
    "mid_nlm_layers_accum": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), _P, _P, _P, _P]),
    "mid_nlm_layers": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), _P, c_void_pp, ctypes.c_int, _P, _P]),
    "mid_nlm_layers_pair_accum": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), _P, _P, _P, _P, _P]),
    "mid_nlm_layers_temporal": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, c_void_pp, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, _P]),
    "mid_bilateral_pair_accum": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), _P, _P, _P, _P]),
    "mid_bilateral_layers_pair_accum": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), _P, _P, _P, _P, _P]),
    "mid_bilateral_temporal": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), c_void_pp, c_void_pp, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, _P]),
    "mid_bilateral_joint": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), ctypes.POINTER(ctypes.c_float), c_void_pp, c_void_pp,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, _P]),
    "mid_nlm_joint": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), ctypes.POINTER(ctypes.c_float), c_void_pp, c_void_pp,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, _P]),
    "mid_atrous_scratch_bytes": (ctypes.c_size_t, [ctypes.POINTER(AtrousParams)]),
    "mid_atrous_joint": (ctypes.c_int, [_P, ctypes.POINTER(AtrousParams), ctypes.POINTER(ctypes.c_float), _P, c_void_pp, ctypes.c_int,
                                        _P, ctypes.c_int, _P, _P]),
    "mid_sequence_atrous_joint": (ctypes.c_int, [_P, ctypes.POINTER(AtrousParams), ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int,
                                                 c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                 ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_atrous_joint_temporal": (ctypes.c_int, [_P, ctypes.POINTER(AtrousParams), ctypes.POINTER(ctypes.c_float), c_void_pp, c_void_pp,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                 _P, _P]),
    "mid_sequence_atrous_joint_temporal": (ctypes.c_int, [_P, ctypes.POINTER(AtrousParams), ctypes.POINTER(ctypes.c_float), c_void_pp,
                                                          ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_atrous_moments": (ctypes.c_int, [_P, ctypes.POINTER(AtrousMomentsParams), ctypes.POINTER(ctypes.c_float), c_void_pp, c_void_pp,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "mid_atrous_variance_scratch_bytes": (ctypes.c_size_t, [ctypes.POINTER(AtrousVarianceParams)]),
    "mid_atrous_variance": (ctypes.c_int, [_P, ctypes.POINTER(AtrousVarianceParams), ctypes.POINTER(ctypes.c_float), _P, _P, c_void_pp,
                                           ctypes.c_int, _P, ctypes.c_int, _P, _P, _P]),
    "mid_sequence_atrous_variance": (ctypes.c_int, [_P, ctypes.POINTER(AtrousVarianceParams), ctypes.POINTER(ctypes.c_float), c_void_pp,
                                                    ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_temporal_accumulate": (ctypes.c_int, [_P, ctypes.POINTER(TemporalAccumParams), ctypes.POINTER(ctypes.c_float), _P, c_void_pp, c_void_pp,
                                               ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mid_sequence_atrous_recursive": (ctypes.c_int, [_P, ctypes.POINTER(TemporalAccumParams), ctypes.POINTER(AtrousVarianceParams),
                                                     ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int, c_void_pp,
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                                     ctypes.POINTER(ctypes.c_float)]),
    "mid_demodulate": (ctypes.c_int, [_P, ctypes.POINTER(AlbedoParams), _P, _P, _P, _P]),
    "mid_modulate": (ctypes.c_int, [_P, ctypes.POINTER(AlbedoParams), _P, _P, _P, ctypes.c_int, _P]),
    "mid_sequence_atrous_recursive_albedo": (ctypes.c_int, [_P, ctypes.POINTER(TemporalAccumParams), ctypes.POINTER(AtrousVarianceParams),
                                                            ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int, c_void_pp,
                                                            c_void_pp, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp,
                                                            ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_firefly_clamp": (ctypes.c_int, [_P, ctypes.POINTER(FireflyParams), _P, _P, _P]),
    "mid_sequence_atrous_recursive_firefly": (ctypes.c_int, [_P, ctypes.POINTER(TemporalAccumParams), ctypes.POINTER(AtrousVarianceParams),
                                                             ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int, c_void_pp,
                                                             c_void_pp, ctypes.c_float, ctypes.POINTER(FireflyParams), ctypes.c_int, ctypes.c_int,
                                                             ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                                             ctypes.POINTER(ctypes.c_float)]),
    "mid_color_bounds": (ctypes.c_int, [_P, ctypes.POINTER(ColorBoundsParams), _P, _P, _P, _P]),
    "mid_temporal_accumulate_clip": (ctypes.c_int, [_P, ctypes.POINTER(TemporalAccumParams), ctypes.POINTER(ctypes.c_float), _P, c_void_pp, c_void_pp,
                                                    ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mid_sequence_atrous_recursive_clip": (ctypes.c_int, [_P, ctypes.POINTER(TemporalAccumParams), ctypes.POINTER(AtrousVarianceParams),
                                                          ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int, c_void_pp,
                                                          c_void_pp, ctypes.c_float, ctypes.POINTER(FireflyParams), ctypes.POINTER(ColorBoundsParams),
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                                          ctypes.POINTER(ctypes.c_float)]),
    "mid_image_metrics_workspace": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "mid_image_metrics": (ctypes.c_int, [_P, ctypes.POINTER(ImageMetricsParams), _P, _P, _P, _P, _P]),
    "mid_image_metrics_derive": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ImageMetricsParams),
                                                ctypes.POINTER(ImageMetricsResult)]),
    "mid_guided_workspace": (ctypes.c_int, [ctypes.POINTER(GuidedParams), ctypes.POINTER(ctypes.c_size_t)]),
    "mid_guided_filter": (ctypes.c_int, [_P, ctypes.POINTER(GuidedParams), _P, _P, _P, _P, ctypes.c_int, _P]),
    "mid_sequence_guided": (ctypes.c_int, [_P, ctypes.POINTER(GuidedParams), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                           c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_median_filter": (ctypes.c_int, [_P, ctypes.POINTER(MedianParams), ctypes.POINTER(ctypes.c_float), _P, c_void_pp, ctypes.c_int, _P,
                                         ctypes.c_int, _P]),
    "mid_sequence_median": (ctypes.c_int, [_P, ctypes.POINTER(MedianParams), ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int, c_void_pp,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_float)]),
    "mid_normalize": (ctypes.c_int, [_P, ctypes.POINTER(NormalizeParams), _P, _P, _P]),
    "mid_unpack_u8": (ctypes.c_int, [_P, _P, ctypes.c_size_t, ctypes.c_int, _P, _P]),
    "mid_pack_u8": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P]),
    "mid_unpack_f16": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P]),
    "mid_pack_f16": (ctypes.c_int, [_P, _P, ctypes.c_size_t, _P, _P]),
    "mid_sequence_nlm": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, ctypes.c_int,
                                        c_void_pp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_nlm_range": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_nlm_range_u8": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_nlm_range_f16": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_bilateral": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int,
                                              c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_nlm_layers": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int,
                                               c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_nlm_layers_temporal": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_bilateral_temporal": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), c_void_pp, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int, ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_bilateral_joint": (ctypes.c_int, [_P, ctypes.POINTER(BilateralParams), ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int,
                                                    c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                                    ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_sequence_nlm_joint": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), ctypes.POINTER(ctypes.c_float), c_void_pp, ctypes.c_int,
                                              c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_pp, ctypes.c_int,
                                              ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mid_nlm_multiframe": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), _P, c_void_pp, ctypes.c_int, _P, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_float)]),
    "mid_pipe_last_timeline": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float),
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_shard_block": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_shard_halo_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_shard_launch_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_comm_unique_id": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint8)]),
    "mid_comm_create": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, ctypes.c_int, c_void_pp]),
    "mid_comm_create_all": (ctypes.c_int, [c_void_pp, ctypes.c_int, c_void_pp]),
    "mid_comm_destroy": (ctypes.c_int, [_P]),
    "mid_comm_abort": (ctypes.c_int, [_P]),
    "mid_comm_reserve": (ctypes.c_int, [_P, ctypes.c_size_t, ctypes.c_int]),
    "mid_comm_rank": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_comm_loopback": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, _P]),
    "mid_comm_last_loopback": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "mid_nlm_temporal_sharded": (ctypes.c_int, [_P, ctypes.POINTER(NlmParams), c_void_pp, ctypes.c_int, ctypes.c_int, c_void_pp, _P]),
    "mid_range_push": (ctypes.c_int, [ctypes.c_char_p]),
    "mid_range_pop": (ctypes.c_int, []),
    "mid_comm_last_exchange": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_float)]),
    "mid_comm_last_timeline": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "mid_comm_last_issue_order": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_size_t]),
    "mid_comm_rccl_info": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_comm_stream_priority": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_comm_boundary_priority": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int)]),
    "mid_image_load": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(Image)]),
    "mid_image_free": (None, [ctypes.POINTER(Image)]),
    "mid_image_load_pinned": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(Image)]),
    "mid_image_free_pinned": (ctypes.c_int, [_P, ctypes.POINTER(Image)]),
    "mid_image_load_f16": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(Image)]),
    "mid_image_save": (ctypes.c_int, [ctypes.c_char_p, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "mid_image_threads": (ctypes.c_int, [ctypes.c_int]),
    "mid_record_begin": (ctypes.c_int, [_P, _P]),
    "mid_record_end": (ctypes.c_int, [_P, _P, c_void_pp]),
    "mid_recording_submit": (ctypes.c_int, [_P, _P]),
    "mid_recording_info": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mid_recording_destroy": (ctypes.c_int, [_P]),
    "mid_timer_create": (ctypes.c_int, [_P, c_void_pp]),
    "mid_timer_destroy": (ctypes.c_int, [_P]),
    "mid_timer_tick": (ctypes.c_int, [_P, _P]),
    "mid_timer_tock": (ctypes.c_int, [_P, _P]),
    "mid_timer_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
}

for _name, (_res, _args) in _SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = the .so does not export what the header declares
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED = tuple(_SIGNATURES)
