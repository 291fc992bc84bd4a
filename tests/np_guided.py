"""Float64 checker of the guided filter (include/mi_denoise.h, section a4o), written from the contract: box sums are plain
cumulative sums over the valid mask, the 3 x 3 systems go to numpy.linalg.solve.  No shift, no fp32 rounding anywhere but the widening
of the inputs: what it returns is the exact answer to about 1e-13 of T (for the conditioning the tests' inputs keep).

    guided(frame, guide, radius, eps) -> dict
        out      (h, w, 4) float64: the contract's output, alpha = the frame's
        T        (h, w, 3): sum_j mean_k|a_k,jc| |I_ij| + mean_k|b_k,c|, the scale of the header's error bound (NaN where passed through)
        abar     (h, w, 3, 3) [guide channel j, output channel c];  bbar (h, w, 3)
        lam_max  (h, w): the largest eigenvalue of Sigma_k (NaN where the window has no model)
        valid    (h, w) bool: the six values finite;  model (h, w) bool: n_k > 0;  filtered (h, w) bool: valid and m_i > 0
        n        (h, w): n_k
"""
import numpy as np


def widen(img):
    """A frame as the kernels read it, then float64: uint8 -> c / 255 correctly rounded to fp32, float16 / float32 exactly."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return (img.astype(np.float32) / np.float32(255)).astype(np.float64)
    return img.astype(np.float32).astype(np.float64)


def box_sum(x, r):
    """Sum of x (h, w, ...) over the window |i|, |j| <= r cut at the image, by two cumulative sums."""
    h, w = x.shape[:2]
    c = np.zeros((h + 1, w + 1) + x.shape[2:], np.float64)
    c[1:, 1:] = x.cumsum(0).cumsum(1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r + 1, h)
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r + 1, w)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def guided(frame, guide, radius, eps):
    P4 = widen(frame)
    G4 = P4 if guide is None else widen(guide)
    assert P4.shape == G4.shape and P4.ndim == 3 and P4.shape[2] == 4
    h, w = P4.shape[:2]
    eps = float(np.float32(eps))
    valid = np.isfinite(P4[..., :3]).all(-1) & np.isfinite(G4[..., :3]).all(-1)
    v = valid.astype(np.float64)
    # (the checker shifts by the valid mean of the whole frame: shift invariance is part of the contract, and the cumulative sums
    # then lose nothing on an HDR or depth-like guide; the kernel's own shift is another one)
    if valid.any():
        sI, sp = G4[..., :3][valid].mean(0), P4[..., :3][valid].mean(0)
    else:
        sI = sp = np.zeros(3)
    I = np.where(valid[..., None], G4[..., :3] - sI, 0.0)
    p = np.where(valid[..., None], P4[..., :3] - sp, 0.0)
    n = box_sum(v, radius)
    model = n > 0
    nn = np.where(model, n, 1.0)
    mu, nu = box_sum(I, radius) / nn[..., None], box_sum(p, radius) / nn[..., None]
    Sig = box_sum(I[..., :, None] * I[..., None, :], radius) / nn[..., None, None] - mu[..., :, None] * mu[..., None, :]
    C = box_sum(I[..., :, None] * p[..., None, :], radius) / nn[..., None, None] - mu[..., :, None] * nu[..., None, :]
    a = np.linalg.solve(Sig + eps * np.eye(3), C)
    b = (nu + sp) - np.einsum("hwjc,hwj->hwc", a, mu + sI)
    a = np.where(model[..., None, None], a, 0.0)
    b = np.where(model[..., None], b, 0.0)
    m = box_sum(model.astype(np.float64), radius)
    filtered = valid & (m > 0)
    mm = np.where(m > 0, m, 1.0)
    abar, bbar = box_sum(a, radius) / mm[..., None, None], box_sum(b, radius) / mm[..., None]
    aabs, babs = box_sum(np.abs(a), radius) / mm[..., None, None], box_sum(np.abs(b), radius) / mm[..., None]
    Iraw = np.where(valid[..., None], G4[..., :3], 0.0)
    fit = np.einsum("hwjc,hwj->hwc", abar, Iraw) + bbar
    out = P4.copy()
    out[..., :3] = np.where(filtered[..., None], fit, P4[..., :3])
    T = np.where(filtered[..., None], np.einsum("hwjc,hwj->hwc", aabs, np.abs(Iraw)) + babs, np.nan)
    lam = np.where(model, np.linalg.eigvalsh(np.where(model[..., None, None], Sig, 0.0))[..., -1], np.nan)
    return {"out": out, "T": T, "abar": abar, "bbar": bbar, "lam_max": lam, "valid": valid, "model": model, "filtered": filtered, "n": n,
            "a": a, "b": b}


TOL_UNITS = 8.0     # the header's bound: |out - exact| <= 8 * 2^-24 * T


def tolerance(ref):
    """The header's bound per pixel and channel (0 where the pixel is passed through: those bits are the input's)."""
    return np.where(ref["filtered"][..., None], TOL_UNITS * 2.0 ** -24 * np.nan_to_num(ref["T"]), 0.0)


def worst_share(got, ref):
    """The largest |got - exact| / tolerance over the filtered pixels' RGB (0 without any), after checking that passed-through pixels
    and alpha hold the input's values (NaN where the input has NaN)."""
    got = np.asarray(got, np.float64)
    f = ref["filtered"]
    np.testing.assert_array_equal(got[..., 3], ref["out"][..., 3])
    np.testing.assert_array_equal(got[~f][..., :3], ref["out"][~f][..., :3])
    if not f.any():
        return 0.0
    err = np.abs(got[f][..., :3] - ref["out"][f][..., :3])
    return float((err / tolerance(ref)[f]).max())
