"""fp64 numpy references for clipping by the global gradient norm: the sum of squares of the rescaled flat bucket, the
norm and the factor, MXNet's Adam update with that factor, and the rounding bound the sum-of-squares launch is held to."""
import math

import numpy as np


def rescales(n, cut, rescale_lo, rescale_hi):
    """r_i: rescale_lo below `cut`, rescale_hi from there on — as fp32 values, which is what the launches are handed"""
    r = np.full(n, float(np.float32(rescale_hi)), np.float64)
    r[:cut] = float(np.float32(rescale_lo))
    return r


def sumsq(grad, cut, rescale_lo, rescale_hi):
    """S = sum_i (g_i r_i)^2 in fp64"""
    g = np.asarray(grad, np.float64)
    x = g * rescales(g.size, cut, rescale_lo, rescale_hi)
    return float(np.sum(x * x))


def norm_and_scale(S, max_norm):
    """(norm, c) in fp64: c = max_norm / (norm + 1e-8), and 1 unless that is below 1"""
    norm = math.sqrt(S)
    c = max_norm / (norm + 1e-8)
    return norm, (c if c < 1.0 else 1.0)


def sumsq_bound(n, n_parts):
    """Relative bound on |sum(parts) - S| for the sum-of-squares launch, derived, not fitted. Every term is non-negative, so relative
    errors do not amplify: a sum of k fp32 roundings of non-negative terms is off by at most about k * 2^-24 relative. One thread of the
    n_parts * 256 adds at most L = ceil(n / (n_parts * 256)) terms in one fp32 chain (its grid-stride four-vectors, four terms each),
    and on top of the chain come the two multiplications of a term (g * r, x * x), six DPP levels of the
    wave sum, the LDS sum of four waves, and slack: 16. (L + 16) * 2^-24."""
    L = -(-n // (n_parts * 256))
    return (L + 16) * 2.0 ** -24


def adam_step(w, g, m, v, t, lr, b1, b2, eps, wd, rescale, clip, c):
    """MXNet's adam_update on fp64 arrays with the global factor c on the rescale: g' = g * (rescale * c) + wd * w, the per-element
    clip if clip >= 0, then the moments and the bias-corrected step"""
    gg = g * (rescale * c) + wd * w
    if clip >= 0:
        gg = np.clip(gg, -clip, clip)
    m = b1 * m + (1 - b1) * gg
    v = b2 * v + (1 - b2) * gg * gg
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    w = w - lr_t * m / (np.sqrt(v) + eps)
    return w, m, v
