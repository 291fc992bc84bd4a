"""Test-only float64 evaluation of the bilateral filter over neighbouring frames (mid_bilateral_pair_accum,
mid_bilateral_layers_pair_accum, mid_bilateral_temporal), written from the contract in include/mi_denoise.h, section a4d:

    w = exp(-0.5 |o|^2 / ss^2) * exp(-0.5 |Gt(p) - Gn(p+o)|^2_rgb / sc^2),   num[p] += w * In(p+o),   den[p] += w

for every tap o = (i, j), |i|, |j| <= R, out-of-image texels vec4(0) in Gn and In; output t = sum over the neighbours
f = max(0,t-k) .. min(n-1,t+k) (and, layered, over the layers) of such sums, divided, magenta where the weights sum to 0.
It shares no code with the kernels (fp32 LDS tiles, exp2 with folded scales): zero-padded 2-D images and one shifted slice per
tap, in torch float64 on the device torch sees (like f64_checker.py) or on the CPU.
"""
import math

import numpy as np
import torch

from f64_checker import device


def decode(a):
    """A frame or guide as the float32 texels the filters read: uint8 -> c/255 (the correctly rounded fp32 quotient), float16
    widened, float32 as it is."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a.astype(np.float32) / np.float32(255.0)
    return a.astype(np.float32)


def _stack(imgs, c, R, dev):
    """[B, h + 2R, w + 2R, c] float64: the images' first c channels, zero-padded by R."""
    x = torch.as_tensor(np.stack([decode(a)[..., :c] for a in imgs]), device=dev).to(torch.float64)
    B, h, w, _ = x.shape
    out = torch.zeros((B, h + 2 * R, w + 2 * R, c), dtype=torch.float64, device=dev)
    out[:, R:R + h, R:R + w] = x
    return out


def pair_sums_many(pairs, R, sigma_s, sigma_c, dev=None):
    """The pair dispatches `pairs` = [(target guide, neighbour guide, neighbour frame)] evaluated together, one shifted slice
    per tap for all of them: (num [B,h,w,4], den [B,h,w]) as float64 torch tensors."""
    dev = device() if dev is None else dev
    h, w = np.asarray(pairs[0][2]).shape[:2]
    gt = _stack([p[0] for p in pairs], 3, 0, dev)
    gn, im = _stack([p[1] for p in pairs], 3, R, dev), _stack([p[2] for p in pairs], 4, R, dev)
    num = torch.zeros((len(pairs), h, w, 4), dtype=torch.float64, device=dev)
    den = torch.zeros((len(pairs), h, w), dtype=torch.float64, device=dev)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            q = gn[:, R + j:R + j + h, R + i:R + i + w]
            d2 = ((gt - q) ** 2).sum(-1)
            wt = math.exp(-0.5 * (i * i + j * j) / float(sigma_s) ** 2) * torch.exp(-0.5 * d2 / float(sigma_c) ** 2)
            num += im[:, R + j:R + j + h, R + i:R + i + w] * wt[..., None]
            den += wt
    return num, den


def pair_sums(target_guide, neighbour_guide, neighbour, R, sigma_s, sigma_c, dev=None):
    """One pair dispatch: (num [h,w,4], den [h,w]) as float64 torch tensors."""
    num, den = pair_sums_many([(target_guide, neighbour_guide, neighbour)], R, sigma_s, sigma_c, dev)
    return num[0], den[0]


def normalize(num, den):
    out = num / den[..., None]
    zero = den == 0
    if bool(zero.any()):
        out[zero] = torch.tensor([1.0, 0.0, 1.0, 1.0], dtype=torch.float64, device=out.device)
    return out.cpu().numpy()


def window(n, t, k):
    return range(max(0, t - k), min(n - 1, t + k) + 1)


def bilateral_temporal(frames, k, R, sigma_s, sigma_c, layers=None, first=0, count=None, skip=(), dev=None):
    """Outputs [first, first+count) as float64 [h,w,4] arrays.  layers: None (plain form) or one list of uint8 layers per frame.
    skip: neighbour frames left out of every window (for the tests' own known answers)."""
    dev = device() if dev is None else dev
    n = len(frames)
    count = n - first if count is None else count
    pairs, owner = [], []
    for t in range(first, first + count):
        for f in window(n, t, k):
            if f in skip:
                continue
            for gt, gf in ([(frames[t], frames[f])] if layers is None else zip(layers[t], layers[f])):
                pairs.append((gt, gf, frames[f]))
                owner.append(t - first)
    h, w = np.asarray(frames[0]).shape[:2]
    num = torch.zeros((count, h, w, 4), dtype=torch.float64, device=dev)
    den = torch.zeros((count, h, w), dtype=torch.float64, device=dev)
    if pairs:
        a, b = pair_sums_many(pairs, R, sigma_s, sigma_c, dev)
        idx = torch.as_tensor(owner, device=dev)
        num.index_add_(0, idx, a)
        den.index_add_(0, idx, b)
    return [normalize(num[i], den[i]) for i in range(count)]
