"""Host references of the per-dimension latent statistics (mst_latent_dim_stats, include/mst_hip.h): the accumulator
acc[c][k][d] of {n, sum mu, sum mu^2, sum sigma^2, sum kl_d} per class c and latent dimension d.

dim_stats_ref is the launch restated: a sequential fp64 loop over the batch in ascending order, every fp32 input widened first, the
skip rules of the header. fp32 x fp32 is exact in fp64 and the order is the kernel's, so planes 0-3 are comparable bit for bit; in
plane 4 only the logarithm may differ (by an ulp between two correctly working libraries). dim_stats_vec is the same sums by whole-array
numpy, whose pairwise summation may differ from the loop in the last bits: the two check each other on finite inputs.
Numpy only: the CPU and the GPU tests import it."""
import numpy as np

PLANES = 5


def _counted(mu, sigma, classes, C):
    """[B, Z] bool: the (sample, dimension) terms that count"""
    mu, sigma, classes = np.asarray(mu, np.float32), np.asarray(sigma, np.float32), np.asarray(classes)
    ok = np.isfinite(mu) & np.isfinite(sigma) & (sigma != 0)
    return ok & ((classes >= 0) & (classes < C))[:, None]


def kl_terms(mu, sigma):
    """kl_d = 0.5 (sigma^2 + mu^2 - 1 - log sigma^2) per element in fp64 on the fp32 values widened (loss.py:8-12, no epsilon), the
    operations in the order written"""
    m, s = np.asarray(mu, np.float32).astype(np.float64), np.asarray(sigma, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s2 = s * s
        return 0.5 * (s2 + m * m - 1.0 - np.log(s2))


def dim_stats_ref(mu, sigma, classes, C):
    """-> fp64 [C, 5, Z]: one launch on a zeroed accumulator"""
    mu, sigma = np.asarray(mu, np.float32), np.asarray(sigma, np.float32)
    B, Z = mu.shape
    ok, kl = _counted(mu, sigma, classes, C), kl_terms(mu, sigma)
    acc = np.zeros((C, PLANES, Z), np.float64)
    for b in range(B):
        c = int(classes[b])
        for d in range(Z):
            if not ok[b, d]:
                continue
            m, s = np.float64(mu[b, d]), np.float64(sigma[b, d])
            acc[c, 0, d] += 1.0
            acc[c, 1, d] += m
            acc[c, 2, d] += m * m
            acc[c, 3, d] += s * s
            acc[c, 4, d] += kl[b, d]
    return acc


def dim_stats_vec(mu, sigma, classes, C):
    """the same sums from whole-array numpy (a second formulation: masks and np.sum instead of a loop)"""
    mu64, s64 = np.asarray(mu, np.float32).astype(np.float64), np.asarray(sigma, np.float32).astype(np.float64)
    ok, kl = _counted(mu, sigma, classes, C), kl_terms(mu, sigma)
    acc = np.zeros((C, PLANES, mu64.shape[1]), np.float64)
    for c in range(C):
        w = ok & (np.asarray(classes) == c)[:, None]
        for k, v in enumerate((np.ones_like(mu64), mu64, mu64 * mu64, s64 * s64, kl)):
            acc[c, k] = np.where(w, v, 0.0).sum(0)
    return acc


def abs_kl_sums(mu, sigma, classes, C):
    """-> fp64 [C, Z]: sum of |kl_d| over the counted terms of a cell, what plane 4's tolerance is relative to"""
    ok, kl = _counted(mu, sigma, classes, C), kl_terms(mu, sigma)
    out = np.zeros((C, np.asarray(mu).shape[1]), np.float64)
    for c in range(C):
        out[c] = np.where(ok & (np.asarray(classes) == c)[:, None], np.abs(kl), 0.0).sum(0)
    return out


def abs_sums(mu, sigma, classes, C):
    """-> fp64 [C, 5, Z]: sum of |term| per cell and plane (two summation orders of the same terms differ by at most
    (terms - 1) 2^-53 of it each)"""
    mu64, s64 = np.asarray(mu, np.float32).astype(np.float64), np.asarray(sigma, np.float32).astype(np.float64)
    ok, kl = _counted(mu, sigma, classes, C), kl_terms(mu, sigma)
    out = np.zeros((C, PLANES, mu64.shape[1]), np.float64)
    for c in range(C):
        w = ok & (np.asarray(classes) == c)[:, None]
        for k, v in enumerate((np.ones_like(mu64), np.abs(mu64), mu64 * mu64, s64 * s64, np.abs(kl))):
            out[c, k] = np.where(w, v, 0.0).sum(0)
    return out


def planted(rng, B, Z, C, pad=3):
    """inputs of a kernel case: mu, sigma as fp32 [B, Z + pad] whose pad columns hold NaN (a read past Z poisons the sums), classes
    int32 [B]; among them, wherever the shape has room, a negative sigma, sigma == 0, a NaN mu, an inf sigma, a class of -1 and a class
    of C. -> (mu_padded, sigma_padded, classes)"""
    mu = np.full((B, Z + pad), np.nan, np.float32)
    sg = np.full((B, Z + pad), np.nan, np.float32)
    mu[:, :Z] = rng.standard_normal((B, Z)).astype(np.float32)
    sg[:, :Z] = np.exp(rng.uniform(-1.5, 1.0, (B, Z))).astype(np.float32)
    sg[:, :Z] *= np.where(rng.random((B, Z)) < 0.25, -1.0, 1.0).astype(np.float32)  # negative sigma: only sigma^2 is used
    classes = rng.integers(0, C, B).astype(np.int32)
    cells = [(b, d) for b in range(B) for d in range(Z)]
    picks = [cells[i] for i in rng.permutation(len(cells))[:min(4, len(cells) // 4)]]  # (at most a quarter of a small case)
    for (b, d), what in zip(picks, ("zero", "nan_mu", "inf_sigma", "neg_zero")):
        if what == "zero":
            sg[b, d] = 0.0
        elif what == "neg_zero":
            sg[b, d] = -0.0
        elif what == "nan_mu":
            mu[b, d] = np.nan
        else:
            sg[b, d] = np.inf
    if B >= 5:
        rows = rng.permutation(B)[:2]
        classes[rows[0]], classes[rows[1]] = -1, C
    return mu, sg, classes
