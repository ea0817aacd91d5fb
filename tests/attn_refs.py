"""A plain fp64 reference of key-row attention (mst_attn_keysoftmax_fwd / _bwd, mst_attn_qkv_fwd; no GPU, no library), the
tolerance every output element is held to, the launch decision restated, and the table of cases that reaches every launch form
(mst_attn_fwd_form / mst_attn_bwd_form in include/mst_hip.h).

The operation (csrc/attention.hip's header; the kernels are in attention_fwd.hip / attention_bwd.hip, their tiles in attention.hpp), per (batch b, head h), on the 16-bit-rounded operands:
    x[k, q] = K[k] . Q[q]                      t[k, q] = fl32(fl32(x * scale) + madd[k]),   madd = 0, or -1e9 for a padded key
    P[k, :] = softmax over q of t[k, :]        out[q]  = sum_k P[k, q] V[k]                 (queries q < q_limit only)
    dV[k] = sum_q P dO[q]     dP[k, q] = dO[q] . V[k]     delta[k] = sum_q P dP     g = scale P (dP - delta)
    dK[k] = sum_q g Q[q]      dQ[q] = sum_k g K[k]        (the fp32 add differentiated as the identity, as autograd does)
The fp32 step is the one the reference model really has: it is why a padded key row is uniform while |x * scale| < 32 and a
few-hot row beyond (fl32(x * scale - 1e9) lands on another multiple of 64). Everything else here is fp64.

A case carries the launch form it is meant for; tests/test_attn_refs_cpu.py asks the library's own decision for it and checks
that the table reaches every form the decision can return."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

BF, FP = torch.bfloat16, torch.float16
DTYPES = (BF, FP)
DT_NAME = {BF: "bf16", FP: "fp16"}
MODES = ("real", "big")
SENTINEL = 7.0
MASK_VALUE = -1e9

FWD_PATHS = ("resident-3", "resident-2", "chunked", "fused", "stream")
BWD_PATHS = ("resident", "stream+chunked-dq", "stream")


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------ the launch decision, restated
LDS_CU = 160 * 1024
LONE_RED = 16 * 32
ATT16_WAVES = 4
QKV_KC = 64


def lone_row_shape(S, dh):
    return dh <= 16 and S > 32 and S % 32 == 1


def choose_resident(S, n_wg, lds, waves_cu=16, lone=False, max_nw=16, force=None):
    """waves per workgroup of a resident kernel, 0 when the sequence does not fit (csrc/attention.hip choose_resident)"""
    if force == "stream" or lds > LDS_CU - 1024:
        return 0
    NB = cdiv(S, 32) - (1 if lone else 0)
    by_grid = cdiv(n_wg, 256)
    best, best_score = 0, 0.0
    for nw in range(1, min(max_nw, NB) + 1):
        wgs = waves_cu // nw
        if wgs * lds > LDS_CU:
            wgs = LDS_CU // lds
        wgs = min(wgs, by_grid)
        if wgs < 1:
            continue
        score = (wgs * nw) * (NB / (nw * cdiv(NB, nw)))
        if score >= best_score:
            best, best_score = nw, score
    return best


def res_lds_fwd(dh, S, tiles):
    SP = cdiv(S, 32) * 32
    return tiles * SP * (dh + 8) * 2 + 5 * SP * 4 + LONE_RED * 4


def res_lds_bwd(dh, S):
    SP = cdiv(S, 32) * 32
    return 2 * SP * (dh + 8) * 2 + 6 * SP * 4 + LONE_RED * 4


def res_max_waves(dh):
    return 8 if dh == 64 else 16


def fwd_form(B, S, H, dh, q_limit=0, fused=False, force=None):
    """what ops.attn_fwd_form returns, decided here from the shape (a restatement: the tests hold it against the library's)"""
    n_wg, NB = B * H, cdiv(S, 32)
    ql = q_limit if 0 < q_limit < S else S
    res = lambda path, nw, lds, lone=0: dict(path=path, waves=nw, lds=lds, lone=int(lone), grid_stats=0, grid_out=0)  # noqa: E731
    if fused and dh == 32:
        lds = res_lds_fwd(32, S, 3)
        nw = choose_resident(S, n_wg, lds, 16, False, force=force)
        if nw >= NB and nw >= 6 and (H * dh) % QKV_KC == 0:
            return res("fused", nw, lds)
    lone = lone_row_shape(S, dh) and ql >= S
    waves_cu = 4 * ATT16_WAVES if dh == 16 else 16
    for tiles, path in ((3, "resident-3"), (2, "resident-2")):
        lds = res_lds_fwd(dh, S, tiles)
        nw = choose_resident(S, n_wg, lds, waves_cu, lone, force=force)
        if nw:
            return res(path, nw, lds, lone)
    if not lone and dh >= 32 and NB % 2 == 0:
        lds, maxw = res_lds_fwd(dh, S, 1), res_max_waves(dh)
        nw = choose_resident(S, n_wg, lds, maxw, False, maxw, force=force)
        if nw and NB <= 2 * nw:
            return res("chunked", nw, lds)
    return dict(path="stream", waves=4, lds=0, lone=0, grid_stats=cdiv(S, 128), grid_out=cdiv(ql, 128))


def bwd_form(B, S, H, dh, q_limit=0, force=None):
    """what ops.attn_bwd_form returns"""
    n_wg, NB = B * H, cdiv(S, 32)
    ql = q_limit if 0 < q_limit < S else 0
    sparse = int(0 < ql <= 32)
    lone = lone_row_shape(S, dh) and not sparse
    lds = res_lds_bwd(dh, S)
    nw = choose_resident(S, n_wg, lds, 4 * ATT16_WAVES if dh == 16 else res_max_waves(dh), lone, res_max_waves(dh), force=force)
    if nw:
        return dict(path="resident", waves=nw, lds=lds, sparse=sparse, lone=int(lone), dq_chunks=0, dq_waves=0)
    if dh == 32 and NB <= 32:
        nc = 1
        while nc <= 4 and NB % nc == 0:
            lds_q = 2 * (NB * 32 // nc) * (dh + 8) * 2 + 6 * NB * 32 * 4
            if lds_q <= 150 * 1024:
                return dict(path="stream+chunked-dq", waves=4, lds=lds_q, sparse=sparse, lone=0, dq_chunks=nc, dq_waves=8)
            nc *= 2
    return dict(path="stream", waves=4, lds=0, sparse=sparse, lone=0, dq_chunks=0, dq_waves=0)


# ------------------------------------------------------------------------------------------ the reference and its bound
U32 = 2.0 ** -24                        # unit roundoff of fp32
UT = {BF: 2.0 ** -8, FP: 2.0 ** -11}    # unit roundoff of the activation type (8 and 11 significand bits, the hidden one included)
# absolute rounding error below the smallest normal. fp16: subnormals are 2^-24 apart. bf16 shares fp32's exponent range: what is
# lost is what fp32 itself loses when a v_exp result or a product falls below 2^-126 and is flushed
ETA = {BF: 2.0 ** -126, FP: 2.0 ** -25}
# v_exp_f32 and v_log_f32 (what fast_exp2, __expf and __logf compile to) are specified to 1 ulp of their fp32 result, 2^-23 relative.
# That figure cannot be measured without the hardware; it is taken with a factor of 2. What CAN be measured on the CPU is the error
# their ARGUMENTS bring, formed in fp32 as the kernels form them: test_attn_refs_cpu.py runs that emulation (sk2, ck2, one fma,
# numpy's float32 exp2) against the fp64 probabilities and finds the worst relative error of P at 0.022 (real) and 0.010 (big) of
# the rho derived below, whose counted terms (S / 2 additions, a rescale per tile) are worst cases the data does not reach. rho is some
# 1e-5: two orders below the activation type's rounding, which decides the bound.
EPS_EXP = 2.0 * 2.0 ** -23
EPS_LOG = 2.0 * 2.0 ** -23


def scale_of(dh):
    """the kernels' a.scale: 1 / sqrt(dh) in fp32 (a power of two at head sizes 16 and 64)"""
    return float(np.float32(1.0) / np.sqrt(np.float32(dh)))


def logits32(x, scale, valid):
    """t = fl32(fl32(x * scale) + madd): the one fp32 step of the reference model, returned in fp64"""
    madd = np.where(valid, np.float32(0.0), np.float32(MASK_VALUE)).astype(np.float32)
    return ((x.astype(np.float32) * np.float32(scale)).astype(np.float32) + madd[:, None]).astype(np.float32).astype(np.float64)


def round_to(a, dtype):
    """round an fp64 array to the activation type and back"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dtype).double().numpy()


def head_ref(K, Q, V, valid, dO, q_limit, dh, dtype=None, mut=None, emulate=None):
    """One (batch, head): K, Q, V, dO fp64 [S, dh], valid bool [S]. -> dict of the results (out [S, dh] with rows >= q_limit zero,
    lse0 / lse1 / delta [S], dV / dK / dQ [S, dh]) and, when dtype is given, of the tolerance of every element (b_out, b_lse,
    b_delta, b_dV, b_dK, b_dQ; see bound notes below).

    mut: one of the wrong results the tests must see refused (MUTATIONS). emulate: an activation type — round where the kernels round
    (logits to fp32, P and g to that type before they become MFMA operands, results to the type): the error a correct kernel shows."""
    S = K.shape[0]
    scale = scale_of(dh)
    ql = q_limit if 0 < q_limit < S else S
    if mut == "q_limit_off_by_one":
        ql = min(S, ql + 1) if ql < S else S - 1
    if mut == "kq_swapped":
        K, Q = Q, K
    if mut == "wrong_scale":
        scale = scale_of(64 if dh != 64 else 32)
    dO = dO.copy()
    dO[ql:] = 0.0
    x = K @ Q.T                                         # [k, q]
    if emulate is not None:
        x = x.astype(np.float32).astype(np.float64)    # (the accumulator's final rounding; the order of the additions is the bound's)
    t = logits32(x, scale, valid)
    if mut == "padded_uniform":
        t = np.where(valid[:, None], t, MASK_VALUE)
    if mut == "padded_excluded":
        t = np.where(valid[:, None], t, -np.inf)
    if mut == "softmax_over_keys":
        m = t.max(0, keepdims=True)
        e = np.exp(t - m)
        P = e / e.sum(0, keepdims=True)
        m, l = t.max(1), np.exp(t - t.max(1)[:, None]).sum(1)
    else:
        m = t.max(1)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(t - m[:, None])
        l = e.sum(1)
        if mut == "ragged_zero_rows":  # the rows of the last 32-row tile beyond S counted as queries with x = 0
            t0 = logits32(np.zeros((S, 1)), scale, valid)[:, 0]
            l = l + (cdiv(S, 32) * 32 - S) * np.exp(t0 - m)
        l = np.where(l > 0, l, 1.0)
        P = e / l[:, None]
    logl = np.log(l)
    Pm = P
    if emulate is not None:
        Pm = round_to(P, emulate)
    elif mut == "p_rounded_bf16":
        Pm = round_to(P, BF)
    Po = Pm
    if mut == "drop_tile":       # one 32-row tile missing from every sum over the partner axis
        Po = Pm.copy()
        Po[:32] = 0.0
    out = Po.T @ V
    out[ql:] = 0.0
    Pv = Pm
    if mut == "drop_tile":
        Pv = Pm.copy()
        Pv[:, :32] = 0.0
    dV = Pv @ dO
    dP = V @ dO.T                                       # [k, q]
    delta = (P * dP).sum(1) if emulate is None else (V * dV).sum(1)
    dl = np.roll(delta, 1) if mut == "delta_shifted" else delta
    G = dP - dl[:, None]
    g = scale * P * G
    gm = round_to(g, emulate) if emulate is not None else g
    gk = gq = gm
    if mut == "drop_tile":
        gk, gq = gm.copy(), gm.copy()
        gk[:, :32] = 0.0
        gq[:32] = 0.0
    dK, dQ = gk @ Q, gq.T @ K
    if mut == "kq_swapped":
        dK, dQ = dQ, dK
    r = dict(out=out, lse0=m, lse1=logl, delta=delta, dV=dV, dK=dK, dQ=dQ)
    if emulate is not None:
        for k in ("out", "dV", "dK", "dQ"):
            r[k] = round_to(r[k], emulate)
    if dtype is None or mut is not None or emulate is not None:
        return r
    # ---- the bound. Every term is a unit roundoff times the fp64 sum of absolute values of what is summed; the counts are read off
    # the tile functions of csrc/attention.hpp and named where they enter.
    u, uT, eta = U32, UT[dtype], ETA[dtype]
    SP, NT = cdiv(S, 32) * 32, cdiv(S, 32)
    unp = valid.astype(np.float64)
    aK, aQ, aV, adO = np.abs(K), np.abs(Q), np.abs(V), np.abs(dO)
    # x: dh products accumulated in fp32 by dh / 16 chained MFMAs (the lone row: dh fmaf in a lane), any order: dh u sum|K||Q|,
    # doubled because MFMA accumulation need not round every addition the IEEE way (as gemm_bound, wgrad_bound). A padded key's
    # -1e9 swallows it (|x scale| < 32) or x is an exact integer (`big` mode), so there it is zero.
    ex = 2.0 * dh * u * (aK @ aQ.T) * unp[:, None]
    d = t - m[:, None]
    tabs = np.abs(t) * unp[:, None]
    ml = np.abs(m + logl) * unp
    # the exponential's argument, natural units. Fast form exp2(fma(x, sk2, ck2)): sk2 = fl(scale fl(log2 e)) 2 u |t|, ck2 =
    # fl(fl(-(m + logl)) fl(log2 e)) 3 u |m + logl|, the fma's rounding u |d - logl|. Exact form exp2(fl(fl(fl(t - m) - logl) fl(log2 e))):
    # u |d| + 3 u |d - logl| (a padded key takes only this one; its t - m is a small multiple of 64, exact).
    dl_ = np.abs(d - logl[:, None])
    e_arith = u * np.maximum(2.0 * tabs + 3.0 * ml[:, None] + dl_, np.abs(d) + 3.0 * dl_)
    # lse = m + logl as the kernels hold it. Statistics sweep: fast form exp2(fma(x, c, -m2)) 2 u |t| + u (|t| + |m|) <= 4 u max|t|,
    # exact form 3 u max|d|; v_exp once per term; at most one rescale per tile and one merge of the lane halves, each an
    # exponential and two roundings; S / 2 in-lane additions + NT + 2 merges; m = fl(m2 fl(ln 2)) 2 u |m|; __logf = v_log * fl(ln 2).
    e_stat = u * np.maximum(4.0 * tabs.max(1), 3.0 * np.abs(d).max(1))
    b_lse = (scale * ex.max(1) + e_stat + (NT + 1) * (EPS_EXP + 2.0 * u) + EPS_EXP + (S / 2.0 + NT + 2) * u + 2.0 * u * np.abs(m) * unp
             + (EPS_LOG + 2.0 * u) * np.abs(logl))
    rho = scale * ex + e_arith + EPS_EXP + b_lse[:, None]     # relative error of P in the fp32 register
    wP = P * (rho + uT * (1.0 + rho)) + eta                   # absolute error of P once rounded to T (fp16: the subnormal step)
    acc = 2.0 * SP * u                                        # SP terms accumulated by the MFMAs (the rows beyond S are zeros)
    fin = lambda b, ref: b * (1.0 + uT) + uT * np.abs(ref) + eta  # noqa: E731  (the result rounded to T)
    b_out = fin(wP.T @ aV + acc * (P.T @ aV), out)
    b_out[ql:] = 0.0
    b_dVacc = wP @ adO + acc * (P @ adO)
    # delta = V . dV from the fp32 dV accumulator (delta_from_dv): dh fmaf + the lane halves' sum
    b_delta = (aV * b_dVacc).sum(1) + 2.0 * (dh + 1) * u * (aV * np.abs(dV)).sum(1)
    # dP - delta: the MFMA accumulator starts at -delta (dh products + 1)
    e_dp = 2.0 * (dh + 1) * u * (aV @ adO.T + np.abs(delta)[:, None]) + b_delta[:, None]
    # P scale: the fast form adds fl(log2 scale) (v_log, 2.5 at head size 32) to ck2, one more rounding of |ck2|; the exact one multiplies
    rho_b = rho + u * (ml[:, None] + 4.0) + EPS_LOG
    e_g = scale * P * (np.abs(G) * (rho_b + u) + e_dp)
    w_g = e_g + uT * (np.abs(g) + e_g) + eta                  # g rounded to T before it becomes an MFMA operand
    r.update(b_out=b_out, b_lse=b_lse, b_delta=b_delta, b_dV=fin(b_dVacc, dV), b_dK=fin(w_g @ aQ + acc * (np.abs(g) @ aQ), dK),
             b_dQ=fin(w_g.T @ aK + acc * (np.abs(g).T @ aK), dQ), rho=rho)
    return r


MUTATIONS = ("drop_tile", "ragged_zero_rows", "wrong_scale", "padded_excluded", "softmax_over_keys", "padded_uniform", "delta_shifted",
             "q_limit_off_by_one", "kq_swapped", "p_rounded_bf16")
RESULTS = ("out", "lse", "dV", "dK", "dQ", "delta")


def attn_ref(K, Q, V, valid, dO, q_limit, dtype=None, mut=None, emulate=None):
    """K, Q, V, dO fp64 [B, S, H, dh], valid bool [B, S] -> the results and bounds of head_ref stacked: out / dV / dK / dQ (and their
    b_) [B, S, H, dh], lse0 / lse1 / delta (b_lse, b_delta) [B, H, S], lse = lse0 + lse1"""
    B, S, H, dh = K.shape
    heads = [[head_ref(K[b, :, h], Q[b, :, h], V[b, :, h], valid[b], dO[b, :, h], q_limit, dh, dtype, mut, emulate) for h in range(H)]
             for b in range(B)]
    r = {}
    for k in heads[0][0]:
        a = np.array([[heads[b][h][k] for h in range(H)] for b in range(B)])   # [B, H, S(, dh | S)]
        r[k] = a.transpose(0, 2, 1, 3) if (a.ndim == 4 and k != "rho") else a
    r["lse"] = r["lse0"] + r["lse1"]
    return r


# ------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """One launch: the shape, the layout, the key masks of its batch elements, and the forms it is meant for."""
    id: str
    B: int
    S: int
    H: int
    dh: int
    fwd: str                      # path of FWD_PATHS the forward launch must take
    bwd: str                      # path of BWD_PATHS the backward launch must take
    fw: int = 0                   # waves per workgroup the forward / backward must report (0: not part of what the case is about)
    bw: int = 0
    q_limit: int = 0
    fused: bool = False           # forward through mst_attn_qkv_fwd
    force: str = None             # MST_ATTN_PATH
    layout: str = "plain"         # plain: ld_qkv = 3 D, offsets (0, D, 2 D), ld_out = ld_dout = D. pad: ld_qkv = ld_dqkv = 3 D + 8 (pad
    #                               columns NaN on input), ld_out = D + 8, ld_dout = D + 16 (fused: ld_x = D + 8, ld_w = D + 16). perm: pad
    #                               with the sections at (2 D, 0, D)
    masks: tuple = ("full",)      # per batch element, cycled: full | mid (a prefix ending mid-tile) | tile (a prefix that leaves the last
    #                               tile wholly padded) | all (every key padded) | holes
    lone: int = 0                 # the lone-row value both directions must report (backward: unless sparse)
    dq_chunks: int = 0

    @property
    def D(self):
        return self.H * self.dh

    @property
    def offs(self):
        D = self.D
        return (2 * D, 0, D) if self.layout == "perm" else (0, D, 2 * D)

    @property
    def lds(self):
        """ld_qkv (= ld_dqkv), ld_out, ld_dout, ld_x, ld_w"""
        D = self.D
        return (3 * D, D, D, D, D) if self.layout == "plain" else (3 * D + 8, D + 8, D + 16, D + 8, D + 16)

    @property
    def sparse(self):
        return int(0 < self.q_limit <= 32 and self.q_limit < self.S)

    def valid(self, mode="real"):
        """bool [B, S]: the key masks (a fused call in `big` mode: no padded key, see operands)"""
        S, NB = self.S, cdiv(self.S, 32)
        v = np.ones((self.B, S), dtype=bool)
        if self.fused and mode == "big":
            return v
        for b in range(self.B):
            kind = self.masks[b % len(self.masks)]
            if kind == "mid":
                n = S - 13 if (S - 13) % 32 else S - 14
                assert 0 < n < S and n % 32 != 0
                v[b, n:] = False
            elif kind == "tile":
                assert NB >= 2
                v[b, 32 * (NB - 1) - 7:] = False
            elif kind == "all":
                v[b] = False
            elif kind == "holes":
                v[b, 3::5] = False
                v[b, S // 2:S // 2 + 9] = False
            else:
                assert kind == "full", kind
        return v


_ALL = ("full", "mid", "tile", "all")
CASES = (
    # ---- head size 32: the three-tile resident forward and the resident backward (one block; ragged; nine blocks, one ragged)
    Case("d32-res3-s64", 4, 64, 1, 32, "resident-3", "resident", masks=("full", "mid", "all", "holes")),
    Case("d32-res3-s100-ql1", 2, 100, 2, 32, "resident-3", "resident", q_limit=1, layout="pad", masks=("full", "mid")),
    Case("d32-res3-s100-ql2", 2, 100, 2, 32, "resident-3", "resident", q_limit=2, layout="perm", masks=("tile", "full")),
    Case("d32-res3-s257-ql33", 2, 257, 2, 32, "resident-3", "resident", q_limit=33, layout="pad", masks=_ALL),
    Case("d32-res3-s257-ql129", 1, 257, 2, 32, "resident-3", "resident", q_limit=129, masks=("mid",)),
    Case("d32-res3-s100-qlS-1", 1, 100, 2, 32, "resident-3", "resident", q_limit=99, masks=("holes",)),
    Case("d32-res3-s100-qlS", 1, 100, 2, 32, "resident-3", "resident", q_limit=100, layout="perm", masks=("mid",)),
    Case("d32-res3-s100-qlS+5", 1, 100, 2, 32, "resident-3", "resident", q_limit=105, masks=("tile",)),
    # ---- the fused projection and its boundaries (6..16 row blocks)
    Case("d32-s160-notfused", 2, 160, 2, 32, "resident-3", "resident", fused=True, masks=("full", "mid")),
    Case("d32-fused-s161", 2, 161, 2, 32, "fused", "resident", fw=6, fused=True, layout="perm", masks=("full", "mid")),
    Case("d32-fused-s200-ql31", 2, 200, 2, 32, "fused", "resident", fused=True, q_limit=31, layout="pad", masks=("tile", "holes")),
    Case("d32-fused-s512", 1, 512, 2, 32, "fused", "resident", fw=16, fused=True, masks=("mid",)),
    Case("d32-s544-notfused", 1, 544, 2, 32, "resident-3", "resident", fw=16, fused=True, masks=("mid",)),  # 17 blocks on 16 waves forward
    # ---- head size 32: two-tile forward; chunked forward + dQ in two chunks; streaming
    Case("d32-res2-s609", 1, 609, 2, 32, "resident-2", "resident", masks=("mid",), layout="pad"),
    Case("d32-res2-s640-ql32", 2, 640, 1, 32, "resident-2", "resident", q_limit=32, masks=("full", "tile")),
    Case("d32-res-bwd-s864", 1, 864, 1, 32, "resident-2", "resident", masks=("holes",)),
    Case("d32-chunk-s865", 1, 865, 2, 32, "chunked", "stream+chunked-dq", dq_chunks=2, masks=("mid",), layout="perm"),
    Case("d32-chunk-s896-ql33", 2, 896, 1, 32, "chunked", "stream+chunked-dq", dq_chunks=2, q_limit=33, masks=("full", "tile")),
    Case("d32-chunk-s1000", 1, 1000, 1, 32, "chunked", "stream+chunked-dq", dq_chunks=2, masks=("all",)),
    Case("d32-chunk-s1024-ql1", 1, 1024, 1, 32, "chunked", "stream+chunked-dq", dq_chunks=2, q_limit=1, masks=("holes",)),
    Case("d32-stream-s897-ql31", 1, 897, 2, 32, "stream", "stream", q_limit=31, masks=("mid",), layout="pad"),
    Case("d32-stream-s928-ql129", 3, 928, 1, 32, "stream", "stream", q_limit=129, masks=("full", "tile", "all")),
    # ---- forced streaming at small S: dQ in one chunk; the XCD remap (batch a multiple of 8) and its absence (3)
    Case("d32-forced-s70", 3, 70, 2, 32, "stream", "stream+chunked-dq", dq_chunks=1, force="stream", masks=_ALL, layout="perm"),
    Case("d32-forced-s70-ql1", 2, 70, 2, 32, "stream", "stream+chunked-dq", dq_chunks=1, force="stream", q_limit=1, masks=("full", "mid")),
    Case("d32-forced-b8-s200", 8, 200, 2, 32, "stream", "stream+chunked-dq", dq_chunks=1, force="stream", masks=_ALL + ("holes",)),
    Case("d16-forced-b16-s161-ql31", 16, 161, 1, 16, "stream", "stream", force="stream", q_limit=31, masks=_ALL, layout="pad"),
    Case("d64-forced-b3-s100", 3, 100, 1, 64, "stream", "stream", force="stream", masks=("mid", "full", "holes")),
    Case("d64-stream-b8-s513-ql2", 8, 513, 1, 64, "stream", "stream", q_limit=2, masks=("full", "mid", "full", "tile")),
    # ---- head size 16: the lone row (33, 65, 257; 1025 on two tiles), three and two tiles, streaming, and resident forward with
    # streaming backward (S 1313..1376)
    Case("d16-lone-s33", 2, 33, 2, 16, "resident-3", "resident", lone=1, masks=("full", "mid")),
    Case("d16-lone-s65-ql32", 2, 65, 2, 16, "resident-3", "resident", q_limit=32, masks=("full", "mid"), layout="perm"),
    Case("d16-lone-s257", 2, 257, 2, 16, "resident-3", "resident", lone=1, masks=("mid", "all"), layout="pad"),
    Case("d16-s960", 1, 960, 1, 16, "resident-3", "resident", masks=("holes",)),
    Case("d16-lone-s1025", 1, 1025, 2, 16, "resident-2", "resident", lone=1, masks=("mid",)),
    Case("d16-s1312", 1, 1312, 1, 16, "resident-2", "resident", masks=("tile",)),
    Case("d16-s1313", 1, 1313, 1, 16, "resident-2", "stream", lone=1, masks=("mid",)),
    Case("d16-s1376", 1, 1376, 1, 16, "resident-2", "stream", masks=("full",)),
    Case("d16-stream-s1377", 1, 1377, 1, 16, "stream", "stream", masks=("mid",)),
    Case("d16-s544", 1, 544, 2, 16, "resident-3", "resident", fw=16, masks=("mid",)),                  # 17 blocks on 16 waves forward
    # ---- head size 64: three tiles to 352, two to 512, streaming beyond; backward with two blocks on a wave from S 288
    Case("d64-res3-s100", 2, 100, 1, 64, "resident-3", "resident", masks=("full", "mid"), layout="perm"),
    Case("d64-res3-s288", 1, 288, 2, 64, "resident-3", "resident", bw=8, masks=("mid",)),               # 9 blocks on 8 waves: uneven
    Case("d64-res3-s352-ql2", 1, 352, 1, 64, "resident-3", "resident", q_limit=2, masks=("tile",)),
    Case("d64-res2-s353", 1, 353, 1, 64, "resident-2", "resident", masks=("mid",), layout="pad"),
    Case("d64-res2-s512", 1, 512, 1, 64, "resident-2", "resident", masks=("holes",)),
    Case("d64-stream-s513-ql129", 1, 513, 2, 64, "stream", "stream", q_limit=129, masks=("mid",)),
    # ---- the grid decides the wave count: more than 1024 workgroups let several share a CU
    Case("d16-grid-s170", 33, 170, 32, 16, "resident-3", "resident", fw=6, bw=3, masks=("full", "mid", "full")),    # 6 blocks: backward on 3 waves
)
"""No admissible shape reaches a second form of the same launch. Two forms the host code can name are never reached (checked against
mst_attn_bwd_form / mst_attn_fwd_form over S = 1..1500 by test_attn_refs_cpu.py): the chunked dQ in 4 chunks (2 chunks always fit
once the sequence has at most 32 blocks), and the chunked forward at head size 64 (it needs at most 16 blocks, which the two-tile
form already takes)."""
CASE = {c.id: c for c in CASES}


def form_calls(c, dtype=BF):
    """-> (positional arguments of ops.attn_fwd_form, of ops.attn_bwd_form) for a case"""
    ldq, ldo, lddo, ldx, ldw = c.lds
    fwd = (dtype, c.B, c.S, c.H, c.dh, *c.offs, ldq, ldo, c.q_limit, c.fused, ldx if c.fused else 0, ldw if c.fused else 0)
    bwd = (dtype, c.B, c.S, c.H, c.dh, *c.offs, ldq, lddo, ldq, c.q_limit)
    return fwd, bwd


def check_forms(c, f, b):
    """what the case states about its forms, against the dicts of ops.attn_fwd_form / attn_bwd_form (or fwd_form / bwd_form): a list
    of disagreements, empty when the launch takes the plan the case is meant for"""
    bad = []
    for name, got, want in (("forward path", f["path"], c.fwd), ("backward path", b["path"], c.bwd), ("dQ chunks", b["dq_chunks"], c.dq_chunks),
                            ("sparse", b["sparse"], c.sparse)):
        if got != want:
            bad.append(f"{name} {got!r}, meant for {want!r}")
    lone_f = c.lone if not (0 < c.q_limit < c.S) else 0
    lone_b = c.lone if (not c.sparse and b["path"] == "resident") else 0
    if f["lone"] != lone_f or b["lone"] != lone_b:
        bad.append(f"lone row forward {f['lone']} backward {b['lone']}, meant for {lone_f} / {lone_b}")
    if c.fw and f["waves"] != c.fw:
        bad.append(f"forward waves {f['waves']}, meant for {c.fw}")
    if c.bw and b["waves"] != c.bw:
        bad.append(f"backward waves {b['waves']}, meant for {c.bw}")
    return bad


# ------------------------------------------------------------------------------------------ operands
BIG_INT = 14        # `big` mode: K and Q are integers in [-14, 14] (exact in bf16 and fp16; every x exact in fp32)
BIG_C = 128         # head size 32, padded keys: K[k] = c e_i with |c| <= 128, so x = c Q[q, i] takes 29 values per key


@functools.lru_cache(maxsize=None)
def good_multipliers():
    """head size 32 (scale not a power of two): the c in 16..128 for which no c j scale, |j| <= 14, lies within 0.5 of a rounding
    boundary 32 + 64 n of fl32(. - 1e9): there fl32(fl32(x scale) - 1e9) and the kernels' fmaf(x, scale, -1e9) cannot differ"""
    j = np.arange(-BIG_INT, BIG_INT + 1, dtype=np.float64)
    return tuple(c for c in range(16, BIG_C + 1) if boundary_distance(c * j * scale_of(32)).min() > 0.5)


def boundary_distance(ts):
    """distance of every x * scale to the nearest 32 + 64 n"""
    r = (np.asarray(ts, dtype=np.float64) - 32.0) % 64.0
    return np.minimum(r, 64.0 - r)


def _seed(c, dtype, mode):
    return [CASES.index(c), DTYPES.index(dtype), MODES.index(mode), 20261]


@functools.lru_cache(maxsize=None)
def operands(cid, dtype, mode):
    """The case's operands as CPU tensors, deterministic (shared by the tests: leave them unchanged): qkv [B S, ld_qkv], dout
    [B S, ld_dout] (rows >= q_limit of every sample zero), keymask uint8 [B, S]; the fused call's x [B S, ld_x], W [3 D, ld_w], bias fp32
    [3 D] instead of qkv. Pad columns hold NaN: the kernels must never read them.
    real: unit-scale normal K, Q, V, dO (fused: x ~ N(0, 1), W ~ N(0, 1 / D), bias ~ 0.2 N(0, 1)).
    big: K and Q integers in [-14, 14] — logits with a standard deviation near 70, exact in fp32, so padded keys' |x scale| spans
    several multiples of 64 and a padded row is few-hot, not uniform; at head size 32 a padded key is c e_i with c from
    good_multipliers(). V and dO as in real mode. Fused, big: x integers in [-3, 3], W four entries of +-1 / +-2 per row, integer
    bias — qkv is exact in the activation type and must come out bit for bit; such a case has no padded key (asserted)."""
    c = CASE[cid]
    rng = np.random.default_rng(_seed(c, dtype, mode))
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    ldq, ldo, lddo, ldx, ldw = c.lds
    valid = c.valid(mode)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dtype)  # noqa: E731

    def padded(a, ld):
        full = torch.full((a.shape[0], ld), float("nan"), dtype=dtype)
        full[:, :a.shape[1]] = t(a)
        return full

    dO = rng.standard_normal((B, S, D))
    if 0 < c.q_limit < S:
        dO[:, c.q_limit:] = 0.0
    o = dict(keymask=torch.from_numpy(valid.astype(np.uint8)), dout=padded(dO.reshape(B * S, D), lddo))
    if c.fused:
        if mode == "big":
            assert valid.all()
            x = rng.integers(-3, 4, (B * S, D)).astype(np.float64)
            W = np.zeros((3 * D, D))
            for r in range(3 * D):
                W[r, rng.choice(D, 4, replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], 4)
            bias = rng.integers(-2, 3, 3 * D).astype(np.float64)
        else:
            x = rng.standard_normal((B * S, D))
            W = rng.standard_normal((3 * D, D)) / math.sqrt(D)
            bias = 0.2 * rng.standard_normal(3 * D)
        o.update(x=padded(x, ldx), W=padded(W, ldw), bias=torch.from_numpy(bias).float())
        return o
    if mode == "big":
        K = rng.integers(-BIG_INT, BIG_INT + 1, (B, S, H, dh)).astype(np.float64)
        Q = rng.integers(-BIG_INT, BIG_INT + 1, (B, S, H, dh)).astype(np.float64)
        if dh == 32:
            good = np.array(good_multipliers(), dtype=np.float64)
            for b, k in zip(*np.nonzero(~valid)):
                K[b, k] = 0.0
                K[b, k, np.arange(H), rng.integers(0, dh, H)] = rng.choice(good, H) * rng.choice([-1.0, 1.0], H)
    else:
        K, Q = rng.standard_normal((B, S, H, dh)), rng.standard_normal((B, S, H, dh))
    V = rng.standard_normal((B, S, H, dh))
    qkv = np.zeros((B * S, 3 * D))
    for a, off in zip((K, Q, V), c.offs):
        qkv[:, off:off + D] = a.reshape(B * S, D)
    o["qkv"] = padded(qkv, ldq)
    return o


def sections(c, qkv, dout):
    """K, Q, V, dO fp64 [B, S, H, dh] out of the (16-bit) qkv and dout tensors of a case"""
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    q, d = qkv.double().numpy(), dout.double().numpy()
    K, Q, V = (q[:, off:off + D].reshape(B, S, H, dh) for off in c.offs)
    return K, Q, V, d[:, :D].reshape(B, S, H, dh)


def qkv_ref(c, o, dtype):
    """the fused call's projection: -> (x W^T + bias fp64 [B S, 3 D], its bound). fp32 accumulation of D products and the bias in any
    order, doubled for the MFMAs (gemm_bound's reasoning), then the rounding to the activation type"""
    D = c.D
    x, W, b = o["x"][:, :D].double().numpy(), o["W"][:, :D].double().numpy(), o["bias"].double().numpy()
    ref = x @ W.T + b
    S_abs = np.abs(x) @ np.abs(W).T + np.abs(b)
    return ref, 2.0 * (D + 1) * U32 * S_abs * (1.0 + UT[dtype]) + UT[dtype] * np.abs(ref) + ETA[dtype]


def reference_on(c, qkv, dout, dtype, mode="real", **kw):
    """attn_ref on the sections of given qkv / dout tensors (the fused call: the qkv the launch itself wrote)"""
    K, Q, V, dO = sections(c, qkv, dout)
    return attn_ref(K, Q, V, c.valid(mode), dO, c.q_limit, dtype, **kw)


@functools.lru_cache(maxsize=None)
def references(cid, dtype, mode):
    """results and bounds of a case that is not a fused call (computed once, shared: leave unchanged)"""
    c, o = CASE[cid], operands(cid, dtype, mode)
    assert not c.fused
    return reference_on(c, o["qkv"], o["dout"], dtype, mode)


def padded_boundary_margin(c, qkv, dout):
    """the smallest distance of a PADDED key's x * scale to a rounding boundary 32 + 64 n (inf without padded keys)"""
    K, Q, _, _ = sections(c, qkv, dout)
    valid, best = c.valid(), np.inf
    for b, k in zip(*np.nonzero(~valid)):
        ts = np.einsum("hd,qhd->hq", K[b, k], Q[b]) * scale_of(c.dh)
        best = min(best, float(boundary_distance(ts).min()))
    return best
