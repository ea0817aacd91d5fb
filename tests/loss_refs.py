"""Plain fp64 references of the loss launches (no GPU, no library), the tolerance every output element is held to, and the tables of
cases that reach every launch form: mst_sigmoid_bce, mst_gemm_sigmoid_bce / _dgrad_ln, mst_softmax_ce, mst_ce_from_probs and
mst_bce_from_probs (csrc/losses.hip, csrc/bce_math.hpp, csrc/gemm_bce.hpp; forms: mst_sigmoid_bce_form / mst_gemm_sigmoid_bce_form).

SIGMOID + BCE (loss.py:27-80), per element on a 16-bit logit x with label y in {0, 1}:
    p = 1 / (1 + e^-x)      s = (1 - ls) y + ls / 2      bce = -(s log(1e-12 + p) + (1 - s) log(1e-12 + (1 - p)))
    where y == 0 and down-weighting is on: bce <- w_b bce^2, w_b = n_pos / (n_neg + 1e-12) over the sample
    loss[b] = mean over the sample's T * P elements      dlogits = d(sum_b loss_b) / dx * gscale
The reference value is that formula in fp64 — EXCEPT for x > 9, where the project keeps the reference model's own fp32 behaviour
(bce_math.hpp: fl(1 - p) no longer resolves the small probability): there the reference value is the formula stepped through in numpy
float32 in bce_exact's order (exact32), and the tolerance is the spread of that evaluation when the hardware exp / rcp results move by
the ulps they may (TR_ULPS), plus the roundings behind them.

THE HARDWARE ASSUMPTION, stated once. bce_math.hpp: "raw v_exp_f32 / v_rcp_f32 / v_log_f32 (1 ulp)", and __expf / __logf / __frcp_rn
compile to them. So every transcendental result is taken to be within 1 ulp of the true function of its fp32 argument; nobody here has
measured that, so it is taken with a factor of 2 (E_TR = 2 * 2^-23 relative, TR_ULPS = 2), as tests/attn_refs.py takes it. One thing
more is assumed: the reciprocal of a power of two is exact (rcp(1) = 1, rcp(2) = 1/2) and so is log2 of one — without it no logit
beyond 16.7 would have a defined gradient (p = 1 - 2^-24 instead of 1 turns log(1e-12 + 0) into log(6e-8)).

BOUNDS (u = 2^-24; E = E_TR). A 16-bit store of a value known to err costs half an ulp of the type at |ref| + err, plus err. The fp32
terms, read off the kernels:
  in the fast domain [-16, 9] (bce_fast): t = exp2(-c |x|): 2 u |x| + E;  q = rcp(1 + t): u + E + rel(t) t;  p = q or t q;
      log q: (E + 2 u) |log q| + rel(q);  log of the smaller: that + u |.|;  bce: three roundings and s's two;  gradient p - s.
      bce_fast drops the 1e-12 epsilons the reference value has: + 1e-12 / p and 1e-12 / (1 - p) on the logarithms and the gradient.
  below -16 (bce_exact against fp64): e^-x: 2 u |x| + E;  1 + e: u;  rcp: E;  fl(1 - p): u absolute;  the two logarithms, the two
      reciprocals and the products as they come, every term on absolute values.
  above 9 (bce_exact against exact32): the spread over exp moved by 0, +-TR_ULPS and rcp by 0, +-1 .. +-TR_ULPS ulps (not where the
      argument is 1), plus (E + 6 u) on the logarithms' and reciprocals' terms.
  down-weighting: w's division and the products of 2 w bce dbce and w bce^2, errors multiplied out on absolute values.
  dlogits: 1 / (T P) and two products, 4 u;  loss[b]: the sum of the element bounds / n + n u sum|bce| / n for a sum in ANY order (the
      partial sums meet in atomics) + 4 u |loss|.
Where bce is tiny against its own error — y == 0, down-weighting on and x beyond 12 (log(fl(1 - p)) moves by 1 / k when 1 - p is k
ulps) or x below -10 (log q cannot resolve 1e-7) — the gradient's bound is many times its rounding. An element whose bound exceeds
four times half an ulp of the output at the reference value is WIDE; the operands keep them at or below 1 % of any output
(tests/test_loss_refs_cpu.py asserts it from the reference alone).

SOFTMAX + CE (model.py:256, loss.py:15-23): fp64 softmax over V; loss[b] = (1 / T) sum_t -log p[label] (label != 0); dlogits =
(p - onehot) (label != 0) / T * gscale; pad columns zero up to min(roundup4(V), ldd). tok_parts: sum -log max(p[label], 1e-10), and
three exact counts (label is the arg-max; among the top_k; label != 0) with ties to the lower index, computed on the 16-bit values.
  e = exp(x - max): u |d| + 2 u |d| + E;  the row sum over ceil(V / 64) + 6 additions;  1 / sum: u;  p: 2 u more;  log: E + 2 u.

No constant here was chosen after looking at a GPU result."""
import functools
import os
import sys
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_refs as G  # noqa: E402
import rowblock_refs as R  # noqa: E402

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF, FP)
DT_NAME = {BF: "bf16", FP: "fp16", F32: "fp32"}
SENTINEL = 7.0
F = np.float32

U = 2.0 ** -24
E_TR = 2.0 * 2.0 ** -23     # relative error of one v_exp / v_rcp / v_log result: 1 ulp as bce_math.hpp states it, doubled; NOT measured
TR_ULPS = 2                 # the same in ulps, for the fp32-stepped evaluation
MANT = {BF: 8, FP: 11, F32: 24}          # significand bits, the hidden one included
EMIN = {BF: -126, FP: -14, F32: -126}    # exponent of the smallest normal
FAST_LO, FAST_HI = -16.0, 9.0            # bce_math.hpp: BCE_FAST_LO, BCE_FAST_HI
CE_MAX_WORKGROUPS = 4096
WIDE_FACTOR, WIDE_CAP = 4.0, 0.01
GSCALE_ODD = float(F(3.3))               # the non-power-of-two loss scale


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def half_ulp(v, dtype):
    """half the spacing of `dtype` at |v| (below the smallest normal: half the subnormal spacing)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** EMIN[dtype])))
    return 2.0 ** (np.maximum(e, EMIN[dtype]) - MANT[dtype])


def store_bound(ref, err, dtype):
    """a value within err of ref, rounded to dtype: half an ulp where it may have landed, plus err"""
    return half_ulp(np.abs(ref) + err, dtype) + err


def is_wide(ref, bound, dtype):
    """a bound above four times the output's rounding at the reference value. A bound below 2^-120 is fp32's own underflow floor under a
    value no type here resolves (a softmax probability of e^-100), not a width"""
    return bound > np.maximum(WIDE_FACTOR * half_ulp(ref, dtype), 2.0 ** -120)


def round_to(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.float32).to(dtype).double().numpy()


def in_domain(x):
    return (x >= FAST_LO) & (x <= FAST_HI)


# ------------------------------------------------------------------------------------------ sigmoid + BCE: the fp32 evaluations
def _nudge(a, k):
    for _ in range(abs(k)):
        a = np.nextafter(a, F(np.inf) if k > 0 else F(-np.inf))
    return a


def _s32(y, ls):
    ls = F(ls)
    return np.where(y != 0, (F(1) - ls) + F(0.5) * ls, F(0.5) * ls).astype(F)


def exact32(x, y, ls, w, dw, de=0, dr=0, true_omp=False):
    """bce_exact in numpy float32, operation by operation -> (p, bce, dbce), after the down-weighting. de / dr: the exp / rcp results
    moved by that many ulps (rcp of exactly 1 stays 1). true_omp: the mistake of taking 1 - p where fl(1 - p) belongs."""
    x, y, w = np.asarray(x, dtype=F), np.asarray(y, dtype=F), np.asarray(w, dtype=F)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        e = _nudge(np.exp(-x).astype(F), de)
        d = F(1) + e
        p = F(1) / d
        p = np.where(d == F(1), p, _nudge(p, dr)).astype(F)
        omp = F(1) - p
        if true_omp:
            omp = (1.0 / (1.0 + np.exp(x.astype(np.float64)))).astype(F)
        ls = F(ls)
        s = ((F(1) - ls) * y + F(0.5) * ls).astype(F)
        lp, lq = np.log(F(1e-12) + p).astype(F), np.log(F(1e-12) + omp).astype(F)
        bce = -(s * lp + (F(1) - s) * lq)
        dbce = -(s * (F(1) / (F(1e-12) + p)) - (F(1) - s) * (F(1) / (F(1e-12) + omp))) * p * omp
        if dw:
            z = y == 0
            dbce = np.where(z, F(2) * w * bce * dbce, dbce)
            bce = np.where(z, w * bce * bce, bce)
    return p.astype(F), bce.astype(F), dbce.astype(F)


def fast32(x, y, ls, w, dw, p_is_q=False):
    """bce_fast in numpy float32 -> (p, bce, dbce)"""
    x, y, w = np.asarray(x, dtype=F), np.asarray(y, dtype=F), np.asarray(w, dtype=F)
    ax = np.abs(x)
    t = np.exp2(F(-1.4426950408889634) * ax).astype(F)
    q = (F(1) / (F(1) + t)).astype(F)
    lbig = F(0.6931471805599453) * np.log2(q).astype(F)
    lsmall = lbig - ax
    pos = x >= 0
    p = np.where(pos | p_is_q, q, t * q).astype(F)
    lp, lq = np.where(pos, lbig, lsmall), np.where(pos, lsmall, lbig)
    s = _s32(y, ls)
    bce = -(s * lp + (F(1) - s) * lq)
    dbce = p - s
    if dw:
        z = y == 0
        dbce = np.where(z, F(2) * w * bce * dbce, dbce)
        bce = np.where(z, w * bce * bce, bce)
    return p, bce.astype(F), dbce.astype(F)


BCE_MISTAKES = ("s_without_half_ls", "n_neg_is_n", "dw_gradient_without_2", "inv_n_is_1_over_T", "gscale_ignored", "neighbour_label",
                "p_of_negative_is_q", "fast_everywhere", "true_1_minus_p")


def bce_mistake_applies(m, x, labels, ls, dw, gscale, want_dl):
    """whether a mistake changes any result of this launch at all (x fp64 [B, T, P])"""
    B, T, P = x.shape
    out = ~in_domain(x)
    return {
        "s_without_half_ls": ls != 0,
        "n_neg_is_n": dw and bool(labels.any()) and not bool(labels.all()),
        "dw_gradient_without_2": dw and want_dl and bool(labels.any()) and not bool(labels.all()),
        "inv_n_is_1_over_T": P > 1,
        "gscale_ignored": gscale != 1.0 and want_dl,
        "neighbour_label": bool((labels != np.roll(labels, -1, axis=2)).any()),
        "p_of_negative_is_q": bool((x < 0).any()),
        "fast_everywhere": bool(out.any()),
        "true_1_minus_p": bool((x > FAST_HI).any()),
    }[m]


def bce_emulate(x, labels, ls, dw, gscale, dtype, order=0, mistake=None):
    """An honest fp32 evaluation that rounds where the kernels round (bce_fast inside the domain, bce_exact outside, fp32 sums in one of
    two orders, results rounded to dtype) — or, with `mistake`, one of the wrong kernels of BCE_MISTAKES.
    -> dict(probs, dlogits fp64 [B, T, P] (16-bit values), loss fp64 [B], npos)"""
    B, T, P = x.shape
    y = labels.astype(F)
    if mistake == "neighbour_label":
        y = np.roll(y, -1, axis=2)
    npos = labels.reshape(B, -1).sum(1).astype(F)
    n = F(T) * F(P)
    nn = n if mistake == "n_neg_is_n" else n - npos
    w = (npos / (nn + F(1e-12))).astype(F).reshape(B, 1, 1) if dw else np.zeros((B, 1, 1), dtype=F)
    x32 = x.astype(F)

    def both(ls_):
        pf, bf_, df = fast32(x32, y, ls_, w, dw, p_is_q=(mistake == "p_of_negative_is_q"))
        pe, be, de_ = exact32(x32, y, ls_, w, dw, true_omp=(mistake == "true_1_minus_p"))
        dom = in_domain(x) | (mistake == "fast_everywhere")
        return np.where(dom, pf, pe), np.where(dom, bf_, be), np.where(dom, df, de_)

    if mistake == "s_without_half_ls":  # s = (1 - ls) y: both branches with the smoothing's second term gone
        xs = x32
        ls32 = F(ls)
        s = ((F(1) - ls32) * y).astype(F)
        pf, _, _ = fast32(xs, y, 0.0, w, False)
        pe, _, _ = exact32(xs, y, 0.0, w, False)
        p = np.where(in_domain(x), pf, pe).astype(F)
        with np.errstate(divide="ignore", invalid="ignore"):
            lp, lq = np.log(F(1e-12) + p), np.log(F(1e-12) + (F(1) - p))
            bce = -(s * lp + (F(1) - s) * lq)
        dbce = p - s
        if dw:
            z = y == 0
            dbce = np.where(z, F(2) * w * bce * dbce, dbce)
            bce = np.where(z, w * bce * bce, bce)
    else:
        p, bce, dbce = both(ls)
    if mistake == "dw_gradient_without_2" and dw:
        dbce = np.where(y == 0, dbce * F(0.5), dbce)
    inv_n = F(1) / (F(T) if mistake == "inv_n_is_1_over_T" else n)
    gs = F(1.0 if mistake == "gscale_ignored" else gscale)
    dl = (dbce.astype(F) * inv_n * gs).astype(F)
    flat = bce.astype(F).reshape(B, -1)
    if order == 0:
        tot = flat.sum(1, dtype=F)                                   # numpy's pairwise order
    else:
        tot = np.array([np.cumsum(r[::-1], dtype=F)[-1] for r in flat], dtype=F)   # one by one, from the end
    loss = (tot * inv_n).astype(np.float64)
    return dict(probs=round_to(p, dtype), dlogits=round_to(dl, dtype), loss=loss, npos=npos.astype(np.int64))


# ------------------------------------------------------------------------------------------ sigmoid + BCE: reference and bound
def bce_ref(x, labels, ls, dw, gscale, dtype):
    """x fp64 [B, T, P] (16-bit logit values), labels uint8 [B, T, P] -> dict: probs, dlogits [B, T, P], loss [B], their bounds b_probs,
    b_dlogits, b_loss, npos int64 [B], and sat (bool: the elements whose reference value is the fp32-stepped one)"""
    B, T, P = x.shape
    u, E = U, E_TR
    y = labels.astype(np.float64)
    ls = float(F(ls))
    gscale = float(F(gscale))
    n = float(T * P)
    npos = labels.reshape(B, -1).astype(np.int64).sum(1)
    w = (npos / ((n - npos) + 1e-12)).reshape(B, 1, 1) if dw else np.zeros((B, 1, 1))
    w = np.broadcast_to(w, x.shape)
    s = (1.0 - ls) * y + 0.5 * ls
    e_s = 2.0 * u * s if ls != 0 else np.zeros_like(s)
    hi, lo = x > FAST_HI, x < FAST_LO

    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        # ---- fp64 values with the epsilons (used where x <= 9)
        p = 1.0 / (1.0 + np.exp(-x))
        omp = 1.0 / (1.0 + np.exp(x))                # 1 - p without cancellation
        lp, lq = np.log(1e-12 + p), np.log(1e-12 + omp)
        bce = -(s * lp + (1.0 - s) * lq)
        dbce = -(s / (1e-12 + p) - (1.0 - s) / (1e-12 + omp)) * p * omp
        ax = np.abs(x)
        # ---- fast domain
        t = np.exp(-ax)
        q = 1.0 / (1.0 + t)
        r_t = 2.0 * u * ax + E
        r_q = u + E + r_t * t
        r_p = np.where(x >= 0, r_q, r_t + r_q + u)
        e_big = (E + 2.0 * u) * np.abs(np.log(q)) + r_q
        e_small = e_big + u * np.abs(np.log(q) - ax)
        e_lp = np.where(x >= 0, e_big, e_small) + 1e-12 / p
        e_lq = np.where(x >= 0, e_small, e_big) + 1e-12 / omp
        e_bce = s * e_lp + (1.0 - s) * e_lq + 3.0 * u * (s * np.abs(lp) + (1.0 - s) * np.abs(lq)) + (e_s + u) * (np.abs(lp) + np.abs(lq))
        e_dbce = r_p * p + e_s + u * np.abs(p - s) + s * 1e-12 / p + (1.0 - s) * 1e-12 / omp
        e_p = r_p * p
        # ---- below the domain: bce_exact, term by term
        r_pl = 2.0 * u * ax + 2.0 * E + u
        e_omp = u + r_pl * p
        a, b = 1e-12 + p, 1e-12 + omp
        r_a = r_pl + 2.0 * u
        e_lp_l = (E + 2.0 * u) * np.abs(lp) + r_a
        e_b = e_omp + u
        e_lq_l = (E + 2.0 * u) * np.abs(lq) + e_b / b
        e_bce_l = (s * e_lp_l + (1.0 - s) * e_lq_l + 3.0 * u * (s * np.abs(lp) + (1.0 - s) * np.abs(lq))
                   + (e_s + u) * (np.abs(lp) + np.abs(lq)))
        t1, t2 = s / a, (1.0 - s) / b
        e_t1 = t1 * (r_a + E + u) + e_s / a
        e_t2 = t2 * (e_b / b + E + u) + (e_s + u) / b
        e_g = e_t1 + e_t2 + u * np.abs(t1 - t2)
        e_dbce_l = e_g * p * omp + np.abs(dbce) * (r_pl + e_omp / omp + 2.0 * u)
        e_p = np.where(lo, r_pl * p, e_p)
        e_bce = np.where(lo, e_bce_l, e_bce)
        e_dbce = np.where(lo, e_dbce_l, e_dbce)
    if dw:  # where y == 0: 2 w bce dbce and w bce^2, the errors multiplied out
        z = y == 0
        d2 = 2.0 * w * bce * dbce
        b2 = w * bce * bce
        e_d2 = 2.0 * w * (e_bce * np.abs(dbce) + np.abs(bce) * e_dbce + e_bce * e_dbce) + 5.0 * u * np.abs(d2)
        e_b2 = w * (2.0 * np.abs(bce) * e_bce + e_bce * e_bce) + 4.0 * u * np.abs(b2)
        dbce, e_dbce = np.where(z, d2, dbce), np.where(z, e_d2, e_dbce)
        bce, e_bce = np.where(z, b2, bce), np.where(z, e_b2, e_bce)

    if hi.any():  # ---- above the domain: the reference's own fp32 evaluation and its spread
        xh, yh, wh, sh = x[hi], labels[hi], w[hi], s[hi]
        p0, b0, d0 = (v.astype(np.float64) for v in exact32(xh, yh, ls, wh, dw))
        sp_p, sp_b, sp_d = np.zeros_like(p0), np.zeros_like(p0), np.zeros_like(p0)
        for de in (-TR_ULPS, 0, TR_ULPS):
            for dr in range(-TR_ULPS, TR_ULPS + 1):
                p1, b1, d1 = exact32(xh, yh, ls, wh, dw, de, dr)
                sp_p, sp_b, sp_d = (np.maximum(sp, np.abs(v.astype(np.float64) - v0)) for sp, v, v0 in
                                    ((sp_p, p1, p0), (sp_b, b1, b0), (sp_d, d1, d0)))
        # the operations behind p, on the unperturbed values: the two logarithms / reciprocals (E each) and the roundings (6 u)
        pr, _, _ = exact32(xh, yh, ls, np.zeros_like(wh), False)
        pr = pr.astype(np.float64)
        ompr = (F(1) - pr.astype(F)).astype(np.float64)
        with np.errstate(divide="ignore"):
            alp, alq = np.abs(np.log(1e-12 + pr)), np.abs(np.log(float(F(1e-12)) + ompr))
        c = E + 6.0 * u
        raw_b = sh * alp + (1.0 - sh) * alq
        raw_d = (sh / (1e-12 + pr) + (1.0 - sh) / (float(F(1e-12)) + ompr)) * pr * ompr
        x_b, x_d = c * raw_b, c * raw_d
        if dw:
            zh = yh == 0
            x_d = np.where(zh, 2.0 * wh * (x_b * raw_d + raw_b * x_d) + 5.0 * u * np.abs(d0), x_d)
            x_b = np.where(zh, wh * 2.0 * raw_b * x_b + 4.0 * u * np.abs(b0), x_b)
        p, bce, dbce = p.copy(), bce.copy(), dbce.copy()
        e_p, e_bce, e_dbce = e_p.copy(), e_bce.copy(), e_dbce.copy()
        p[hi], bce[hi], dbce[hi] = p0, b0, d0
        e_p[hi], e_bce[hi], e_dbce[hi] = sp_p, sp_b + x_b, sp_d + x_d

    dl = dbce / n * gscale
    e_dl = (e_dbce + 4.0 * u * np.abs(dbce)) / n * gscale
    bsum = bce.reshape(B, -1)
    loss = bsum.sum(1) / n
    b_loss = e_bce.reshape(B, -1).sum(1) / n + n * u * np.abs(bsum).sum(1) / n + 4.0 * u * np.abs(loss)
    return dict(probs=p, b_probs=store_bound(p, e_p, dtype), dlogits=dl, b_dlogits=store_bound(dl, e_dl, dtype), loss=loss, b_loss=b_loss,
                npos=npos, sat=hi)


def bce_known(labels, ls, dw, gscale, T, P, dtype):
    """every logit 0, T * P and gscale powers of two: p = 1/2 (rcp(2)), both logarithms -fl(ln 2), dbce = 1/2 - s in fp32, scaled by
    powers of two -> (probs, dlogits) as the kernels must store them bit for bit, and the mask of the dlogits elements that holds for:
    with down-weighting AND smoothing, bce = -(s L + (1 - s) L) of a y == 0 element depends on whether the compiler contracts the sum
    into an fma, so those elements stay with the bound."""
    y = labels.astype(F)
    B = labels.shape[0]
    npos = labels.reshape(B, -1).sum(1).astype(F)
    n = F(T) * F(P)
    w = (npos / ((n - npos) + F(1e-12))).astype(F).reshape(B, 1, 1) if dw else np.zeros((B, 1, 1), dtype=F)
    p, _, dbce = fast32(np.zeros(labels.shape, dtype=F), y, ls, w, dw)
    dl = dbce * (F(1) / n) * F(gscale)
    exact = np.ones(labels.shape, dtype=bool) if not (dw and ls != 0) else (labels != 0)
    return round_to(p, dtype), round_to(dl, dtype), exact


# ------------------------------------------------------------------------------------------ sigmoid + BCE: cases and operands
BCE_MODES = ("real", "sat", "known")
SAT_HI = (17.5, 18.0, 20.0, 24.0, 30.0, 40.0)      # beyond 17.5 p is exactly 1 in fp32: the branches differ visibly in loss[b]
SAT_LO = (-25.0, -26.0, -28.0, -30.0, -32.0, -40.0)  # beyond -25 the 1e-12 epsilons are visible
SAT_ZONE = (13.0, 15.0)                              # the few planted elements whose bound is wide (12 .. 17.4)


@dataclass(frozen=True)
class BceCase:
    id: str
    B: int
    T: int
    P: int
    ld: int                 # of the logits
    ldp: int
    ldd: int
    form: tuple             # (vec, label_bytes, count0, count1, gx) the launch must report
    ls: float = 0.0
    dw: bool = False
    gscale: float = 1.0
    off_p: int = 0          # elements the probs / dlogits base sits behind a 16-byte boundary (4: 8 bytes)
    off_d: int = 0
    decoder: bool = False   # decode.py's call: labels all zero, probs only, npos given, pre_zeroed

    @property
    def modes(self):
        pow2 = lambda v: v > 0 and float(np.log2(v)).is_integer()  # noqa: E731
        return BCE_MODES if pow2(self.T * self.P) and pow2(self.gscale) else BCE_MODES[:2]


BCE_CASES = (
    # 4-wide sweep, labels byte by byte; 7 * 30 = 210 bytes per sample: samples 1 and 2 count their positives byte by byte
    BceCase("p30-bytes", 3, 7, 30, 32, 32, 32, (4, 1, 8, 1, 1), ls=0.1, dw=True, gscale=GSCALE_ODD),
    BceCase("p30-bytes-plain", 3, 7, 30, 32, 32, 32, (4, 1, 0, 0, 1), ls=0.0, dw=False, gscale=1.0),
    # 4-wide, 4-byte label loads (36 % 4 == 0, 36 % 8 != 0); 180 bytes per sample
    BceCase("p36-4byte", 2, 5, 36, 40, 40, 44, (4, 4, 8, 1, 1), ls=0.0, dw=True, gscale=4.0),
    BceCase("p36-4byte-ls", 2, 5, 36, 40, 44, 40, (4, 4, 0, 0, 1), ls=0.1, dw=False, gscale=GSCALE_ODD),
    # 8-wide, two workgroups per sample
    BceCase("p128-wide", 2, 64, 128, 128, 128, 128, (8, 8, 8, 8, 2), ls=0.1, dw=True, gscale=4.0),
    BceCase("p128-wide-plain", 2, 64, 128, 128, 136, 128, (8, 8, 0, 0, 2), ls=0.0, dw=False, gscale=1.0),
    # 4-wide although P % 8 == 0: a leading dimension
    BceCase("p128-ld132", 2, 64, 128, 132, 128, 128, (4, 4, 8, 8, 2), ls=0.0, dw=True, gscale=1.0),
    BceCase("p128-ldd132", 2, 64, 128, 128, 128, 132, (4, 4, 0, 0, 2), ls=0.1, dw=False, gscale=4.0),
    # 4-wide, chosen by a pointer: probs, then dlogits, 8 bytes behind a 16-byte boundary
    BceCase("p128-probs+8", 2, 64, 128, 128, 128, 128, (4, 4, 8, 8, 2), ls=0.1, dw=True, gscale=GSCALE_ODD, off_p=4),
    BceCase("p128-dlogits+8", 2, 64, 128, 128, 128, 128, (4, 4, 0, 0, 2), ls=0.0, dw=False, gscale=4.0, off_d=4),
    # the decoder's call
    BceCase("decoder-t1", 4, 1, 128, 128, 128, 0, (8, 8, 0, 0, 1), decoder=True),
)
BCE_CASE = {c.id: c for c in BCE_CASES}


def _rng(*key):
    return np.random.default_rng([int(k) for k in key] + [20262])


def _name_key(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s))


def _to16(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dtype)


def row_kinds(B, T):
    """`sat` mode, per row [B, T]: 0 every element inside the fast domain, 1 exactly one element outside in this row's GROUP (it sits in
    the group's first row), 2 every element outside. Groups are 8 consecutive rows — both kernels' waves cover 2 to 8 consecutive rows —
    in the cycle (inside, one, outside, alternating rows); samples of fewer than 16 rows are one group each, cycling (one, outside, inside)."""
    k = np.zeros((B, T), dtype=np.int64)
    if T < 16:
        for b in range(B):
            kind = (1, 2, 0)[b % 3]
            if kind == 1:
                k[b, 0] = 1
            else:
                k[b] = kind
        return k
    for b in range(B):
        for g0 in range(0, T, 8):
            kind = ((g0 // 8) + b) % 4
            if kind == 1:
                k[b, g0] = 1
            elif kind == 2:
                k[b, g0:g0 + 8] = 2
            elif kind == 3:
                k[b, g0:g0 + 8:2] = 2
    return k


def sat_values(shape, labels, dw, rng, kinds):
    """the logits of `sat` mode, fp64 [B, T, P]: unit-scale values inside the domain; outside, values of SAT_LO / SAT_HI — a y == 0
    element under down-weighting always from SAT_HI (below -16 its bound would be wide: bce = -log(fl(1 - p)) cannot resolve p), a
    y == 1 element under down-weighting always from SAT_LO, the others from either; the first two lone elements take SAT_ZONE."""
    B, T, P = shape
    x = np.clip(rng.standard_normal(shape), -6.0, 6.0)
    low = rng.random(shape) < 0.5
    if dw:
        low = labels != 0
    val = np.where(low, rng.choice(SAT_LO, shape), rng.choice(SAT_HI, shape))
    x = np.where((kinds == 2)[:, :, None], val, x)
    zone = 0
    for b, t in zip(*np.nonzero(kinds == 1)):
        col = int(rng.integers(0, P))
        if zone < len(SAT_ZONE) and labels[b, t, col] == 0:
            x[b, t, col] = SAT_ZONE[zone]
            zone += 1
        else:
            x[b, t, col] = val[b, t, col]
    return x


@functools.lru_cache(maxsize=None)
def bce_operands(cid, dtype, mode):
    """-> dict(logits [B T, ld] 16-bit with NaN pad columns (a 4-wide sweep loads the pad columns of a ragged row; no result may depend
    on them), labels uint8 [B T, P]); deterministic, shared: leave unchanged"""
    c = BCE_CASE[cid]
    rng = _rng(_name_key(cid), DTYPES.index(dtype), BCE_MODES.index(mode))
    shape = (c.B, c.T, c.P)
    labels = (rng.random(shape) < 0.1).astype(np.uint8)
    if c.decoder:
        labels[:] = 0
    if mode == "known":
        x = np.zeros(shape)
    elif mode == "sat":
        x = sat_values(shape, labels, c.dw, rng, row_kinds(c.B, c.T))
    else:
        x = np.clip(rng.standard_normal(shape), -6.0, 6.0)
    logits = torch.full((c.B * c.T, c.ld), float("nan"), dtype=dtype)
    logits[:, :c.P] = _to16(x.reshape(-1, c.P), dtype)
    return dict(logits=logits, labels=torch.from_numpy(labels.reshape(-1, c.P)))


def bce_reference_on(logits16, labels, c_or_args, dtype):
    """bce_ref on a 16-bit logits tensor [B T, >= P] and labels [B T, P]; c_or_args: anything with B, T, P, ls, dw, gscale"""
    c = c_or_args
    x = logits16[:, :c.P].double().numpy().reshape(c.B, c.T, c.P)
    return bce_ref(x, labels.numpy().reshape(c.B, c.T, c.P), c.ls, c.dw, c.gscale, dtype)


@functools.lru_cache(maxsize=None)
def bce_references(cid, dtype, mode):
    o = bce_operands(cid, dtype, mode)
    return bce_reference_on(o["logits"], o["labels"], BCE_CASE[cid], dtype)


def bce_form_call(c, dtype, base=1 << 20):
    """keyword arguments of ops.sigmoid_bce_form for a case, with plain addresses (`base` stands for any 256-byte aligned allocation)"""
    return dict(dtype=dtype, B=c.B, T=c.T, P=c.P, logits=base, ld_logits=c.ld, labels=2 * base, label_smoothing=c.ls, downweight=c.dw,
                npos=3 * base, loss=4 * base, probs=5 * base + 2 * c.off_p, ldp=c.ldp, dlogits=None if c.decoder else 6 * base + 2 * c.off_d,
                ldd=c.ldd, gscale=c.gscale, pre_zeroed=c.decoder)


def form_tuple(f):
    return (f["vec"], f["label_bytes"], f["count0"], f["count1"], f["gx"])


# ------------------------------------------------------------------------------------------ the fused launches
@dataclass(frozen=True)
class FusedCase:
    id: str
    B: int
    T: int
    P: int
    K: int
    form: tuple             # (BN, column tiles, launches: 0 plain, 1 _dgrad_ln as one launch, 2 as the two)
    ls: float = 0.0
    dw: bool = False
    gscale: float = 4.0
    alpha: float = 1.0
    with_c: bool = True     # the logit gradient is stored
    with_probs: bool = True
    dgrad: bool = False     # through mst_gemm_sigmoid_bce_dgrad_ln (model width = K = 128)
    drop: float = 0.0

    @property
    def modes(self):
        return BCE_MODES

    @property
    def M(self):
        return self.B * self.T


FUSED_CASES = (
    FusedCase("bn128", 2, 64, 128, 64, (128, 1, 0), ls=0.1),
    FusedCase("bn256-dw", 2, 64, 256, 64, (256, 1, 0), dw=True),
    FusedCase("bn256x2-alpha", 2, 64, 512, 64, (256, 2, 0), ls=0.1, alpha=1.5),     # two column tiles share the sample's atomic
    FusedCase("bn128-forward", 2, 64, 128, 64, (128, 1, 0), with_c=False),
    FusedCase("bn128-noprobs", 2, 64, 128, 64, (128, 1, 0), ls=0.1, dw=True, with_probs=False),
    FusedCase("dgrad-one", 2, 64, 128, 128, (128, 1, 1), ls=0.1, dw=True, dgrad=True),
    FusedCase("dgrad-one-drop", 2, 64, 128, 128, (128, 1, 1), dgrad=True, drop=0.2),
    FusedCase("dgrad-two-p256", 2, 64, 256, 128, (256, 1, 2), ls=0.1, dw=True, dgrad=True),
)
FUSED_CASE = {c.id: c for c in FUSED_CASES}
FUSED_SITE, FUSED_SEED_WORD = 9, 77
IND_ALL, IND_ONE = 1, 2      # the last two columns of A: row indicators of `sat` mode


@functools.lru_cache(maxsize=None)
def fused_operands(cid, dtype, mode):
    """x [B (T + 1), K] (the decoder's output: rows 1 .. T of every T + 1 are the launch's), W [P, K], bias fp32 [P], labels; with dgrad
    also Wt [K, P], h (the pre-norm tensor) [B (T + 1), K], gamma, mean, rstd.
    sat: the last two columns of x are row indicators and the matching columns of W carry +-(24 .. 40) / alpha for every pitch (a row
    with the first indicator set lies entirely outside the domain) resp. 28 / alpha for one pitch (the second: one element outside);
    labels of a wholly-outside row follow the sign (y == 1 where the column is negative) under down-weighting."""
    c = FUSED_CASE[cid]
    rng = _rng(_name_key(cid) + 7, DTYPES.index(dtype), BCE_MODES.index(mode))
    B, T, P, K, Sd = c.B, c.T, c.P, c.K, c.T + 1
    x = rng.standard_normal((B * Sd, K))
    W = 0.1 * rng.standard_normal((P, K))
    bias = 0.1 * rng.standard_normal(P)
    labels = (rng.random((B, T, P)) < 0.1).astype(np.uint8)
    if mode == "known":
        x[:], W[:], bias[:] = 0.0, 0.0, 0.0
    if mode == "sat":
        kinds = row_kinds(B, T)
        x[:, K - 2:] = 0.0
        xr = x.reshape(B, Sd, K)
        xr[:, 1:, K - IND_ALL] = (kinds == 2)
        xr[:, 1:, K - IND_ONE] = (kinds == 1)
        neg = rng.random(P) < 0.5
        W[:, K - IND_ALL] = np.where(neg, -32.0, 24.0) / c.alpha
        W[:, K - IND_ONE] = 0.0
        W[int(rng.integers(0, P)), K - IND_ONE] = 28.0 / c.alpha
        if c.dw:
            labels = np.where((kinds == 2)[:, :, None], neg[None, None, :].astype(np.uint8), labels)
    o = dict(x=_to16(x, dtype), W=_to16(W, dtype), bias=torch.from_numpy(bias).float(), labels=torch.from_numpy(labels.reshape(B * T, P)))
    if c.dgrad:
        h = rng.standard_normal((B * Sd, K))
        o["h"] = _to16(h, dtype)
        hf = o["h"].float()
        o.update(Wt=o["W"].t().contiguous(), gamma=torch.from_numpy(1.0 + 0.1 * rng.standard_normal(K)).float(), mean=hf.mean(1),
                 rstd=(hf.var(1, unbiased=False) + 1e-5).rsqrt())
    return o


def phys_rows(c):
    m = np.arange(c.M, dtype=np.int64)
    return (m // c.T) * (c.T + 1) + 1 + m % c.T


def fused_logits_ref(c, o, dtype):
    """the output layer itself: alpha (x W^T + bias) on the remapped rows -> (ref fp64 [M, P], bound): gemm_refs.gemm_bound"""
    A = o["x"][torch.from_numpy(phys_rows(c))].double().numpy()
    Wd, b = o["W"].double().numpy(), o["bias"].double().numpy()
    alpha = float(F(c.alpha))
    ref = (A @ Wd.T + b) * alpha
    S = (np.abs(A) @ np.abs(Wd).T + np.abs(b)) * abs(alpha)
    return ref, G.gemm_bound(SimpleNamespace(c_f32=False, dtype=dtype, K=c.K), ref, S)


def fused_dgrad_ref(c, o, dlogits16, dtype):
    """dX_out and the LayerNorm partial sums of _dgrad_ln on the dlogits the launch wrote: rowblock_refs' GEMM + LayerNorm-backward
    (mask mode 2) stage -> dict(dx=(ref [M, K], bound), dgamma=(ref [K], bound), dbeta=...)"""
    A, Wt = dlogits16.double().numpy(), o["Wt"].double().numpy()
    dy, S = R.gemm_ref(A, Wt, None, 1.0, False, None, False, None, None)
    e = R.gemm_bound(dtype, c.P, dy, S)
    pm = phys_rows(c)
    if c.drop > 0:
        idx = pm.astype(np.uint64)[:, None] * np.uint64(c.K) + np.arange(c.K, dtype=np.uint64)[None, :]
        keep, scale = G.keep_mask(FUSED_SEED_WORD, FUSED_SITE, idx, c.drop)
        k = keep * scale
    else:
        k = np.ones((c.M, c.K))
    pmt = torch.from_numpy(pm)
    return R.ln_bwd_ref(dy, o["h"][pmt].double().numpy(), o["mean"][pmt].double().numpy(), o["rstd"][pmt].double().numpy(),
                        o["gamma"].double().numpy(), k, 2, dtype, e, init=0.0)


# ------------------------------------------------------------------------------------------ softmax + CE
CE_MODES = ("real", "wide", "known")
CE_MISTAKES = ("mean_over_valid", "mask_dropped", "onehot_at_label_plus_1", "ties_to_higher", "topk_le", "pad_not_zeroed")


@dataclass(frozen=True)
class CeCase:
    id: str
    B: int
    T: int
    V: int
    ld: int
    ldd: int
    ldp: int = 0            # 0: V + 3
    gscale: float = 1.0
    top_k: int = 5
    with_probs: bool = True
    with_dl: bool = True
    decoder: bool = False   # labels all zero, probs only, pre_zeroed
    ties: bool = False      # planted exact ties (real mode only)

    @property
    def modes(self):
        return ("real",) if self.ties else CE_MODES

    @property
    def M(self):
        return self.B * self.T

    @property
    def grid(self):
        return min(cdiv(self.M, 4), CE_MAX_WORKGROUPS)

    @property
    def strided(self):
        """the grid-stride loop is taken: more rows than the grid's waves"""
        return self.M > 4 * CE_MAX_WORKGROUPS

    @property
    def zero_end(self):
        return min(roundup(self.V, 4), self.ldd)


CE_CASES = (
    CeCase("v10-pad", 3, 5, 10, 16, 16, gscale=4.0, top_k=5),                    # pad columns 10, 11 zero; 12 .. 15 untouched
    CeCase("v10-ldd10", 3, 5, 10, 16, 10, gscale=GSCALE_ODD, top_k=1),           # ldd clamps the zeroed pad
    CeCase("v293", 8, 65, 293, 296, 300, gscale=4.0, top_k=5),                   # V % 4 != 0, five lane rounds
    CeCase("v293-noprobs", 8, 65, 293, 296, 296, top_k=293, with_probs=False),
    CeCase("v2048", 2, 4, 2048, 2048, 2048, gscale=GSCALE_ODD, top_k=5),
    CeCase("v2048-nodl", 2, 4, 2048, 2056, 0, top_k=1, with_dl=False),
    CeCase("v2", 2, 3, 2, 8, 4, gscale=4.0, top_k=1),
    CeCase("rows16400-stride", 2, 8200, 10, 16, 12, gscale=4.0, top_k=5),        # the grid-stride loop; a workgroup's waves in several strides
    CeCase("rows16405-cross", 5, 3281, 10, 16, 16, gscale=GSCALE_ODD, top_k=10),  # a wave's stride crosses samples
    CeCase("decoder-t1", 4, 1, 293, 296, 0, with_dl=False, decoder=True),       # every row masked
    CeCase("v37-ties", 3, 9, 37, 40, 40, gscale=4.0, top_k=5, ties=True),
)
CE_CASE = {c.id: c for c in CE_CASES}


@functools.lru_cache(maxsize=None)
def ce_operands(cid, dtype, mode):
    """-> dict(logits [M, ld] 16-bit, pad columns NaN (never read), labels int32 [M]).
    real: 2 N(0, 1). wide: uniform over +-80 — probabilities underflow and the label's p is 0; the label is never the row's arg-max
    except in row 1 (there p - 1 cancels and the bound is wide: one element). known: equal logits. A `ties` case plants, in every
    row, entries EQUAL to the label's value on both sides of its index, and entries just above and below it."""
    c = CE_CASE[cid]
    rng = _rng(_name_key(cid) + 13, DTYPES.index(dtype), CE_MODES.index(mode))
    M, V = c.M, c.V
    if mode == "known":
        x = np.full((M, V), 1.25)
    elif mode == "wide":
        x = rng.uniform(-80.0, 80.0, (M, V))
    else:
        x = 2.0 * rng.standard_normal((M, V))
    x = _to16(x, dtype).double().numpy()
    labels = rng.integers(0, V, M)
    labels[::4] = 0            # PAD positions
    if mode == "wide":
        am = x.argmax(1)
        clash = (labels == am) & (labels != 0)
        labels[clash] = (labels[clash] % (V - 1)) + 1
        clash = (labels == am)
        labels[clash & (labels != 0)] = 0
        if M > 1 and V > 2:
            labels[1] = am[1] if am[1] != 0 else 1
    if mode == "wide":   # every second row: the label at the bottom of the range and the arg-max at the top: p[label] = e^-160
        am = x.argmax(1)
        for m in range(0, M, 2 if V > 2 else 1):
            if labels[m] != 0 and labels[m] != am[m]:
                x[m, labels[m]], x[m, am[m]] = -80.0, 80.0
    if c.decoder:
        labels[:] = 0
    if c.ties:
        for m in range(M):
            lab = int(rng.integers(6, V - 6))
            labels[m] = lab if m % 4 else 0
            v = x[m, lab]
            step = float(half_ulp(v, dtype) * 2.0)
            n_eq_lo, n_eq_hi = m % 3, (m // 3) % 3        # equal entries below / above the label's index
            idx_lo = rng.choice(np.arange(0, lab), n_eq_lo + 1, replace=False)
            idx_hi = rng.choice(np.arange(lab + 1, V), n_eq_hi + 1, replace=False)
            x[m, idx_lo[:n_eq_lo]] = v
            x[m, idx_hi[:n_eq_hi]] = v
            x[m, idx_lo[-1]] = v + step                   # just above, below the index
            x[m, idx_hi[-1]] = v - step                   # just below, above the index
        x = _to16(x, dtype).double().numpy()
    logits = torch.full((M, c.ld), float("nan"), dtype=dtype)
    logits[:, :V] = _to16(x, dtype)
    return dict(logits=logits, labels=torch.from_numpy(labels.astype(np.int32)))


def ce_ref(x, labels, c, dtype, mistake=None, emulate=None):
    """x fp64 [M, V] (16-bit values), labels int [M] -> dict(probs [M, V], dlogits [M, V], loss [B], tok (nll sum, arg-max count, top-k
    count, valid count: of ONE launch) and the bounds b_probs, b_dlogits, b_loss, b_nll).
    mistake: one of CE_MISTAKES (a wrong kernel); emulate: an order (0 / 1) — fp32 arithmetic that rounds where the kernel rounds"""
    B, T, V, M = c.B, c.T, c.V, c.M
    u, E = U, E_TR
    gscale = float(F(c.gscale))
    valid = labels != 0
    if mistake == "mask_dropped":
        valid = np.ones_like(valid)
    rows = np.arange(M)
    xl = x[rows, labels]
    if emulate is not None:
        x32 = x.astype(F)
        mx = x32.max(1, keepdims=True)
        with np.errstate(under="ignore"):
            e = np.exp(x32 - mx).astype(F)
            se = (e.sum(1, dtype=F) if emulate == 0 else np.cumsum(e[:, ::-1], axis=1, dtype=F)[:, -1]).astype(F)
            lse = (mx[:, 0] + np.log(se).astype(F)).astype(F)
            p = (e * (F(1) / se)[:, None]).astype(F)
            lpl = (xl.astype(F) - lse).astype(F)
            nll_t = -np.log(np.maximum(np.exp(lpl).astype(F), F(1e-10))).astype(F)
        p, lpl, nll_t = p.astype(np.float64), lpl.astype(np.float64), nll_t.astype(np.float64)
    else:
        mx = x.max(1, keepdims=True)
        e = np.exp(x - mx)
        se = e.sum(1)
        p = e / se[:, None]
        lse = mx[:, 0] + np.log(se)
        lpl = xl - lse
        nll_t = -np.log(np.maximum(np.exp(lpl), 1e-10))
    denom = np.full(B, float(T))
    if mistake == "mean_over_valid":
        denom = np.maximum(valid.reshape(B, T).sum(1), 1).astype(np.float64)
    drow = np.repeat(denom, T)
    loss = (-lpl * valid / drow).reshape(B, T).sum(1)
    onehot = np.zeros((M, V))
    onehot[rows, (labels + 1) % V if mistake == "onehot_at_label_plus_1" else labels] = 1.0
    dl = (p - onehot) * (valid / drow)[:, None] * gscale
    # token metrics on the 16-bit values: entries that beat the label's
    col = np.arange(V)[None, :]
    tie_wins = (col > labels[:, None]) if mistake == "ties_to_higher" else (col < labels[:, None])
    beat = ((x > xl[:, None]) | ((x == xl[:, None]) & tie_wins)).sum(1)
    tv = labels != 0
    in_topk = (beat <= c.top_k) if mistake == "topk_le" else (beat < c.top_k)
    tok = np.array([nll_t[tv].sum(), float(((beat == 0) & tv).sum()), float((in_topk & tv).sum()), float(tv.sum())])
    r = dict(probs=p, dlogits=dl, loss=loss, tok=tok)
    if emulate is not None or mistake is not None:
        if emulate is not None:
            r["dlogits"] = round_to(dl, dtype)
        return r
    # ---- bounds
    d = x - mx
    r_e = 3.0 * u * np.abs(d) + E                               # x - max (u |d|), the product with log2 e (2 u |d|), v_exp
    depth = cdiv(V, 64) + 6
    r_se = (e * r_e).sum(1) / se + depth * u
    r_p = r_e + r_se[:, None] + 3.0 * u
    e_p = r_p * p + 2.0 ** -125                                 # an exponential below 2^-126 is flushed
    gs = (valid / T)[:, None] * gscale
    e_dl = (e_p + 4.0 * u * np.abs(p - onehot)) * gs
    e_lse = (E + 2.0 * u) * np.abs(np.log(se)) + r_se + u * np.abs(lse)
    e_lp = e_lse + u * np.abs(lpl)
    term = np.abs(lpl) * valid / T
    b_loss = ((e_lp * valid / T + 3.0 * u * term).reshape(B, T).sum(1) + T * u * term.reshape(B, T).sum(1))
    # -log max(exp(lp), 1e-10): the exponential's argument errs by e_lp, the two transcendentals by E each, |nll| <= 23.03
    e_nll = e_lp + 3.0 * u * np.abs(lpl) + E + (E + 2.0 * u) * np.abs(nll_t) + u
    waves = 4 * c.grid
    b_nll = e_nll[tv].sum() + (cdiv(M, waves) + 6) * u * np.abs(nll_t[tv]).sum()
    r.update(b_probs=e_p, b_dlogits=store_bound(dl, e_dl, dtype), b_loss=b_loss, b_nll=b_nll)
    return r


def ce_known(c, labels, dtype):
    """equal logits: e = 1, the row sum V, p = fl(1 / V) -> (probs fp32, dlogits as stored) bit for bit: (p - onehot) ((1 / T) gscale),
    every operation in float32 as the kernel has it"""
    M, V = c.M, c.V
    p = np.full((M, V), F(1) * (F(1) / F(V)), dtype=F)
    onehot = np.zeros((M, V), dtype=F)
    onehot[np.arange(M), labels] = 1
    gs = ((labels != 0).astype(F) * (F(1) / F(c.T)) * F(c.gscale)).astype(F)
    return p.astype(np.float64), round_to(((p - onehot) * gs[:, None]).astype(F), dtype)


def ce_mistake_applies(m, x, labels, c):
    pads = (labels == 0)
    if m in ("mean_over_valid", "mask_dropped"):
        return bool(pads.any()) and not bool(pads.all()) if m == "mean_over_valid" else bool(pads.any())
    if m == "onehot_at_label_plus_1":
        return c.with_dl and bool((~pads).any())
    if m == "pad_not_zeroed":
        return c.with_dl and c.zero_end > c.V
    r0, r1 = ce_ref(x, labels, c, BF, emulate=0), ce_ref(x, labels, c, BF, mistake=m, emulate=0)
    return not np.array_equal(r0["tok"][1:], r1["tok"][1:])


@functools.lru_cache(maxsize=None)
def ce_references(cid, dtype, mode):
    c, o = CE_CASE[cid], ce_operands(cid, dtype, mode)
    return ce_ref(o["logits"][:, :c.V].double().numpy(), o["labels"].numpy().astype(np.int64), c, dtype)


# ------------------------------------------------------------------------------------------ the losses on probabilities
PROB_DTYPES = (F32, BF, FP)
PROBS_B, PROBS_T, PROBS_V, PROBS_LDP, PROBS_N = 3, 300, 12, 16, 3000   # the 256- and 1024-thread loops wrap; 3000 % 1024 != 0


@functools.lru_cache(maxsize=None)
def probs_operands(dtype):
    """ce: probs [B T, ldp] (rows of a softmax, pad columns NaN), labels int32 [B T]; bce: probs [B, n] in (0, 1) with a few exact 0
    and 1 entries, labels uint8 [B, n]"""
    rng = _rng(31, PROB_DTYPES.index(dtype))
    z = rng.standard_normal((PROBS_B * PROBS_T, PROBS_V))
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    cp = torch.full((PROBS_B * PROBS_T, PROBS_LDP), float("nan"), dtype=dtype)
    cp[:, :PROBS_V] = torch.from_numpy(p).to(torch.float32).to(dtype)
    cl = rng.integers(0, PROBS_V, PROBS_B * PROBS_T)
    cl[::5] = 0
    bp = rng.uniform(0.02, 0.98, (PROBS_B, PROBS_N))
    bp[:, 7], bp[:, 1500] = 0.0, 1.0
    bl = (rng.random((PROBS_B, PROBS_N)) < 0.1).astype(np.uint8)
    return dict(ce_probs=cp, ce_labels=torch.from_numpy(cl.astype(np.int32)), bce_probs=torch.from_numpy(bp).to(torch.float32).to(dtype),
                bce_labels=torch.from_numpy(bl))


def ce_probs_ref(probs, labels, B, T):
    """probs fp64 [B T, V], labels [B T] -> (loss [B], bound): T logarithms ((E + 2 u) |log p| each), summed in any order, / T"""
    pl = probs[np.arange(B * T), labels]
    term = np.where(labels != 0, -np.log(pl), 0.0).reshape(B, T)
    loss = term.sum(1) / T
    return loss, ((E_TR + 2.0 * U) * np.abs(term)).sum(1) / T + T * U * np.abs(term).sum(1) / T + 2.0 * U * np.abs(loss)


def bce_probs_ref(p, labels, ls, dw):
    """p fp64 [B, n], labels [B, n] -> (loss [B], bound): bce_probs_kernel's operations, every term on absolute values"""
    u, E = U, E_TR
    B, n = p.shape
    y = labels.astype(np.float64)
    ls = float(F(ls))
    s = (1.0 - ls) * y + 0.5 * ls
    e_s = 3.0 * u * s if ls != 0 else np.zeros_like(s)
    la, lb = np.log(1e-12 + p), np.log(1e-12 + (1.0 - p))
    bce = -(s * la + (1.0 - s) * lb)
    # the addends 1e-12f + p and 1e-12f + fl(1 - p) (u each, and the constant's own u where it is all there is), the logarithms
    e_la = (E + 2.0 * u) * np.abs(la) + 2.0 * u
    e_lb = (E + 2.0 * u) * np.abs(lb) + 3.0 * u
    e_bce = s * e_la + (1.0 - s) * e_lb + 3.0 * u * (s * np.abs(la) + (1.0 - s) * np.abs(lb)) + (e_s + u) * (np.abs(la) + np.abs(lb))
    if dw:
        npos = (labels == 1).sum(1).astype(np.float64)
        w = (npos / ((n - npos) + 1e-12))[:, None]
        z = y == 0
        b2 = w * bce * bce
        e_bce = np.where(z, w * (2.0 * np.abs(bce) * e_bce + e_bce ** 2) + 4.0 * u * np.abs(b2), e_bce)
        bce = np.where(z, b2, bce)
    loss = bce.sum(1) / n
    return loss, e_bce.sum(1) / n + n * u * np.abs(bce).sum(1) / n + 2.0 * u * np.abs(loss)
