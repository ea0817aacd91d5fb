"""Plain fp64 references of the class-conditional MMD penalty (csrc/class_mmd.hip; include/mst_hip.h at mst_class_mmd; no GPU, no
library) and the bounds the launch is held to. numpy only. Every reference works on the fp32 inputs widened.

The launch's arithmetic: q_ij = |z_i - z_j|^2 in fp32 by fmaf in ascending d on the fp32 differences, a_ij = q_ij / (2 s2) by one fp32
division, k_ij the fp32 exponential of -a_ij; the counts, w_ij, c_ij = 2 w_ij k_ij / s2, z_j - z_i and every sum over j in fp64. With
u = 2^-24:
  a difference carries u, its square 2u, the Z fused additions of positive terms at most Z u more, the division u: a_ij is off by at most
  (Z + 3) u a_ij, which the exponential turns into the same RELATIVE error of k_ij; the exponential itself adds an ulp = 2u. Rounded up:
      e_ij = u ((Z + 5) a_ij + 4)                                       relative error of k_ij
      |dL_i|    <= sum_j |w_ij| k_ij e_ij + B 2^-53 sum_j |w_ij| k_ij  (the fp64 sum of B terms in any order)
      |dg_i[d]| <= sum_j |c_ij| |z_j[d] - z_i[d]| (e_ij + 2u)
  an fp32 addition: u of the result; a rounding of an fp64 value to fp32: u of the value;
  d(enc_out): (2Z + 2) u sum_j |add_j Wl[j, e]| for the 2Z-term fp32 dot product and its addition to the old value, plus what the
  additions' own errors contribute through |Wl|, plus half an ulp of the activation type at the result.
No free constants."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
ACT_BITS = {"bf16": 8, "fp16": 11}       # significand bits of the activation types
ACT_EMIN = {"bf16": -126, "fp16": -14}   # exponent of the smallest normal


def weights(cl):
    """w_ij = [c_i == c_j] / (n n_{c_i}) - 1 / n^2, fp64 [B, B]; classes are compared, never an index"""
    cl = np.asarray(cl)
    n = float(cl.shape[0])
    same = cl[:, None] == cl[None, :]
    n_c = same.sum(1).astype(np.float64)
    return np.where(same, 1.0 / (n * n_c[:, None]), 0.0) - 1.0 / (n * n)


def mmd_ref(z, cl, s2):
    """z fp32 [B, Z] (no pad columns), cl int [B], s2 the bandwidth as the launch receives it (fp32) ->
    (L_rows [B], g [B, Z], bound_L [B], bound_g [B, Z]) in fp64"""
    z = np.asarray(z, np.float32).astype(np.float64)
    s2 = float(np.float32(s2))
    B, Z = z.shape
    diff = z[None, :, :] - z[:, None, :]           # [i, j, d] = z_j - z_i
    q = (diff * diff).sum(2)
    a = q / (2.0 * s2)
    k = np.exp(-a)
    w = weights(cl)
    wk = w * k
    c = 2.0 * wk / s2
    L_rows = wk.sum(1)
    g = (c[:, :, None] * diff).sum(1)
    e = U * ((Z + 5) * a + 4)
    bound_L = (np.abs(wk) * e).sum(1) + B * U64 * np.abs(wk).sum(1)
    bound_g = (np.abs(c)[:, :, None] * np.abs(diff) * (e + 2 * U)[:, :, None]).sum(1)
    return L_rows, g, bound_L, bound_g


def half_ulp(x, act):
    """half an ulp of the activation type at |x| (at least that of its smallest normal)"""
    ex = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** ACT_EMIN[act])))
    return 2.0 ** (ex - ACT_BITS[act])


def apply_ref(g, bound_g, eps, coef, Wl, dlat_old, denc_old, act):
    """the launch's additions. g, bound_g: mmd_ref's; eps fp32 [B, Z]; coef as the launch receives it (fp32); Wl fp32 [2Z, De];
    dlat_old fp32 [B, 2Z]; denc_old [B, De] the old 16-bit values widened; act 'bf16' / 'fp16' ->
    dict(add [B, 2Z], add_bound, dlat [B, 2Z], dlat_bound, denc [B, De], denc_bound) in fp64"""
    g, eps = np.asarray(g, np.float64), np.asarray(eps, np.float32).astype(np.float64)
    Wl, coef = np.asarray(Wl, np.float32).astype(np.float64), float(np.float32(coef))
    dlat_old, denc_old = np.asarray(dlat_old, np.float32).astype(np.float64), np.asarray(denc_old, np.float64)
    Z = g.shape[1]
    add = np.concatenate([coef * g, coef * g * eps], axis=1)
    # what the kernel's g is off by, scaled as the addition scales it, and the rounding of the addition to fp32
    add_bound = np.concatenate([abs(coef) * bound_g, np.abs(coef * eps) * bound_g], axis=1) + U * np.abs(add)
    dlat = dlat_old + add
    dlat_bound = add_bound + U * (np.abs(dlat) + add_bound)                       # the fp32 addition: u of the result
    prod = add @ Wl                                                              # [B, De]
    absprod = np.abs(add) @ np.abs(Wl)
    pre = add_bound @ np.abs(Wl) + (2 * Z + 2) * U * (absprod + add_bound @ np.abs(Wl))
    denc = denc_old + prod
    pre = pre + U * (np.abs(denc) + pre)                                           # float(old) + sum: u of the result
    denc_bound = pre + half_ulp(np.abs(denc) + pre, act)
    return dict(add=add, add_bound=add_bound, dlat=dlat, dlat_bound=dlat_bound, denc=denc, denc_bound=denc_bound)


CLASS_IDS = (-3, 7, 0, -2147483648, 2147483647)  # what the classes 0 .. C - 1 of planted() are called: any int32 is a class


def planted(rng, B, Z, C, pad=3):
    """inputs with everything the launch has to get right at once: rows padded by `pad` columns that hold NaN (z and eps: [B, Z + pad],
    use [:, :Z]); class ids that are negative and huge; with C >= 2 and B >= 3 a class with a single member (row 0); with B >= 2 two
    identical rows (the last two); with C >= 2 the mean of class 0 shifted by 0.7 in every dimension. -> (z, eps, cl) fp32, fp32, int32"""
    z = np.full((B, Z + pad), np.nan, np.float32)
    eps = np.full((B, Z + pad), np.nan, np.float32)
    z[:, :Z] = rng.standard_normal((B, Z)).astype(np.float32)
    eps[:, :Z] = rng.standard_normal((B, Z)).astype(np.float32)
    idx = rng.integers(0, C, size=B)
    if C >= 2 and B >= 3:
        idx[idx == C - 1] = 0
        idx[0] = C - 1
    if C >= 2:
        z[idx == 0, :Z] += np.float32(0.7)
    if B >= 2:
        z[B - 1] = z[B - 2]
    cl = np.asarray(CLASS_IDS, np.int64)[idx].astype(np.int32)
    return z, eps, cl
