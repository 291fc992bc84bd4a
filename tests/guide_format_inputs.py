"""Inputs of the half / float guide-layer tests (test_bilateral_guide_contract.py on the CPU, test_gpu_bilateral_guide_formats.py
on the GPU): guide layers as a renderer writes them beside an HDR beauty pass, none of which survives quantisation to 8 bits in
[0, 1], and an fp32 restatement of the header's contract for such guides.

The guides: signed "normals" in [-1, 1], HDR "albedo" up to 4, and "depth" with a large offset (7.5) and small local variation.
SIGMA_C = 0.5, so max |g| <= 8 = 16 SIGMA_C: the condition include/mi_denoise.h states for the bilateral tolerance.  The depth
layer is the one that costs precision (|g| / SIGMA_C = 15..16); frames are HDR colours up to 4.
"""
import numpy as np

SIGMA_S, SIGMA_C = 2.0, 0.5
TOL = 1e-5                                         # the project's bilateral tolerance: 1e-5 max(1, |ref|)


def hdr_frames(shape, n, seed=11, translucent=False):
    """n float32 frames of one scene, colours up to 4, some alpha != 1 texels if asked."""
    rng = np.random.default_rng(seed)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([2.0 + 1.8 * np.sin(xx * 0.21), 1.5 + 1.2 * np.cos(yy * 0.17), 3.5 * (xx + yy) / (h + w)], -1)
    out = []
    for _ in range(n):
        f = np.concatenate([np.clip(base * rng.gamma(16.0, 1 / 16.0, (h, w, 1)), 0, 4), np.ones((h, w, 1))], -1).astype(np.float32)
        if translucent:
            f[rng.random((h, w)) < 0.05, 3] = 0.5
        out.append(f)
    return out


def render_layers(shape, n, dtype=np.float32, seed=12):
    """[frame][layer] guides of `dtype` (float32 or float16): normals, albedo, depth; alpha is whatever (it is ignored)."""
    rng = np.random.default_rng(seed)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for f in range(n):
        nrm = np.stack([np.sin(xx * 0.11 + 0.3 * f), np.cos(yy * 0.13), np.sin((xx + yy) * 0.07)], -1)
        nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-3) + rng.normal(0, 0.02, (h, w, 3))
        alb = np.clip(np.stack([2.0 + 1.9 * np.sin(xx * 0.19), 1.0 + np.cos(yy * 0.23 + f), 4.0 * ((xx * 3 + yy * 5) % 32) / 32], -1)
                      + rng.normal(0, 0.05, (h, w, 3)), 0, 4)
        dep = 7.5 + 0.2 * np.stack([np.sin(xx * 0.05 + yy * 0.03), np.cos(xx * 0.04), np.sin(yy * 0.06 + 0.1 * f)], -1) \
            + rng.normal(0, 0.02, (h, w, 3))
        layers = []
        for i, g in enumerate((np.clip(nrm, -1, 1), alb, np.clip(dep, 7.0, 8.0))):
            alpha = np.full((h, w, 1), (1.0, -2.0, 100.0)[i])
            layers.append(np.concatenate([g, alpha], -1).astype(dtype))
        out.append(layers)
    return out


def max_guide_ratio(layers, sigma_c=SIGMA_C):
    return max(float(np.max(np.abs(np.asarray(l, np.float64)[..., :3]))) for ls in layers for l in ls) / sigma_c


def fp32_pair_sums(target_guide, neighbour_guide, neighbour, R, sigma_s, sigma_c):
    """One pair dispatch as the header states it for the kernels, in fp32: a guide value is carried as the fp32 product
    g * sqrt(0.5 log2 e) / sigma_c, the weight is 2^(ks |o|^2 - |difference of the scaled guides|^2), the sums are fp32.
    (num [h,w,4], den [h,w]) float32.  Not the kernels' code: no tiles, no FMA contraction, NumPy's exp2."""
    f32 = np.float32
    sc = f32(np.sqrt(0.5 * 1.4426950408889634) / float(sigma_c))
    ks = f32(-0.5 * 1.4426950408889634 / float(sigma_s) ** 2)
    gt = np.asarray(target_guide).astype(f32)[..., :3] * sc
    h, w = gt.shape[:2]
    gn = np.zeros((h + 2 * R, w + 2 * R, 3), f32)
    gn[R:R + h, R:R + w] = np.asarray(neighbour_guide).astype(f32)[..., :3] * sc
    im = np.zeros((h + 2 * R, w + 2 * R, 4), f32)
    im[R:R + h, R:R + w] = np.asarray(neighbour).astype(f32)
    num, den = np.zeros((h, w, 4), f32), np.zeros((h, w), f32)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            d = gt - gn[R + j:R + j + h, R + i:R + i + w]
            arg = ks * f32(i * i + j * j) - d[..., 0] * d[..., 0] - d[..., 1] * d[..., 1] - d[..., 2] * d[..., 2]
            wt = np.exp2(arg.astype(f32)).astype(f32)
            num += im[R + j:R + j + h, R + i:R + i + w] * wt[..., None]
            den += wt
    return num, den
