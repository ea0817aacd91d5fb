"""A plain fp64 reference of causal attention (mst_attn_causal_fwd / _bwd, csrc/attention_causal.hip; no GPU, no library), the
tolerance every output element is held to, and the table of cases that reaches all 18 kernel instantiations (forward, query-owner
backward, key-owner backward; head sizes 16, 32, 64; bf16 and fp16 — one form per head size, so there is no launch decision).

The operation (include/mst_hip.h), per (batch b, head h), on the 16-bit-rounded operands, scale = fl32(1 / sqrt(dh)):
    logit[q, k] = Q[q] . K[k] * scale     for k <= q and keymask[b, k]; every other pair is excluded, its P exactly 0
    P[q, :] = softmax over k              out[q] = sum_k P[q, k] V[k]
    lse0[q] = max_k logit[q, k]           lse1[q] = log sum_k exp(logit[q, k] - lse0[q])
    dV[k] = sum_q P dO[q]      dP[q, k] = dO[q] . V[k]      delta[q] = sum_k P dP      dS = P (dP - delta)
    dQ[q] = scale sum_k dS K[k]           dK[k] = scale sum_q dS Q[q]
THE CONTRACT FOR A QUERY WITHOUT AN ADMISSIBLE KEY (key 0 masked: the leading queries; a sequence masked entirely): out[q] = 0,
lse0[q] = lse1[q] = -inf, delta[q] = 0, and the query contributes to no gradient (its dQ row is 0). This is what the kernels do — the
forward's running maximum stays -inf, its sum 0, logf(0) = -inf, 1 / l is replaced by 0; the backward admits no pair of that row — and
not what a softmax over an empty set gives in torch (NaN).

Everything here is fp64 but `emulate=`, which rounds where the kernels round."""
import functools
import math
import os
import sys
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_refs import BF, DT_NAME, DTYPES, EPS_EXP, EPS_LOG, ETA, FP, SENTINEL, U32, UT, cdiv, round_to, scale_of  # noqa: E402,F401

BLK = 32
MODES = ("real", "late", "early")
RESULTS = ("out", "lse", "delta", "dQ", "dK", "dV")
MUTATIONS = ("diagonal_excluded", "block_granular_causality", "mask_ignored_in_backward", "drop_block", "stale_rescale",
             "rows_beyond_s_counted", "row_group_swapped", "wrong_scale", "delta_shifted", "kq_swapped", "softmax_over_queries",
             "p_rounded_bf16", "empty_row_nan")


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------ the reference and its bound
def head_ref(Q, K, V, valid, dO, dh, dtype=None, mut=None, emulate=None):
    """One (batch, head): Q, K, V, dO fp64 [S, dh], valid bool [S]. -> dict of the results (out, dQ, dK, dV [S, dh]; lse0, lse1,
    delta [S]) and, when dtype is given, of the tolerance of every element (b_out, b_lse, b_delta, b_dQ, b_dK, b_dV).

    mut: one of the wrong results the tests must see refused (MUTATIONS). emulate: an activation type — round where the kernels
    round (logits and dP to fp32, the forward's exp(t - m) and the backward's P and dS to that type before they become MFMA
    operands, lse to fp32 before the backward adds its planes, results to the type): the error a correct kernel shows."""
    S = Q.shape[0]
    NB, scale = cdiv(S, BLK), scale_of(dh)
    SP = NB * BLK
    if mut == "kq_swapped":
        K, Q = Q, K
    if mut == "wrong_scale":
        scale = scale_of(64 if dh != 64 else 32)
    qi, ki = np.arange(S)[:, None], np.arange(S)[None, :]
    causal = ki <= qi
    if mut == "diagonal_excluded":
        causal = ki < qi
    if mut == "block_granular_causality":
        causal = ki // BLK <= qi // BLK
    adm = causal & valid[None, :]
    has = adm.any(1)
    x = Q @ K.T                                           # [q, k]
    t_all = x * scale
    if emulate is not None:
        t_all = _f32(_f32(x) * scale)
    t = np.where(adm, t_all, -np.inf)
    ms = np.where(has, t.max(1, initial=-np.inf), 0.0)    # (0 stands in on the rows without keys: every e below is 0 there)
    e = np.exp(t - ms[:, None])
    l = e.sum(1)
    if mut == "rows_beyond_s_counted":   # the SP - S keys behind the sequence counted with logit 0 by the queries of the last block
        last = has & (np.arange(S) >= BLK * (NB - 1))
        ms = np.where(last, np.maximum(ms, 0.0), ms)
        e = np.exp(t - ms[:, None])
        l = e.sum(1) + np.where(last, (SP - S) * np.exp(-ms), 0.0)
    ls = np.where(has, l, 1.0)
    logl = np.log(ls)
    P = e / ls[:, None]
    if mut == "softmax_over_queries":
        mq = np.where(adm.any(0), t.max(0, initial=-np.inf), 0.0)
        eq = np.exp(t - mq[None, :])
        P = eq / np.where(adm.any(0), eq.sum(0), 1.0)[None, :]

    # ---- forward
    Pf = P
    if emulate is not None:
        Pf = round_to(e, emulate) / ls[:, None]
    if mut == "p_rounded_bf16":
        Pf = round_to(P, BF)
    if mut == "drop_block":
        Pf = Pf.copy()
        Pf[:, :BLK] = 0.0
    if mut == "stale_rescale":   # the part of out gathered before the diagonal block keeps the maximum it was gathered under
        before = ki < BLK * (qi // BLK)
        m_prev = np.where(before, t, -np.inf).max(1, initial=-np.inf)
        m_prev = np.where(np.isfinite(m_prev), m_prev, ms)
        Pf = np.where(before, np.exp(t - m_prev[:, None]), e) / ls[:, None]
    if mut == "row_group_swapped":
        Pp, Vp = np.zeros((S, SP)), np.zeros((SP, dh))
        Pp[:, :S], Vp[:S] = Pf, V
        out = Pp[:, np.arange(SP) ^ 4] @ Vp
    else:
        out = Pf @ V
    lse0, lse1 = np.where(has, ms, -np.inf), np.where(has, logl, -np.inf)
    if mut == "empty_row_nan":
        for q in np.nonzero(~has)[0]:
            out[q] = V[:q + 1].mean(0)
        lse0, lse1 = np.where(has, lse0, np.nan), np.where(has, lse1, np.nan)

    # ---- backward
    Pb = P
    if mut == "mask_ignored_in_backward":
        Pb = np.where(causal & has[:, None], np.exp(np.where(causal, t_all, -np.inf) - (ms + logl)[:, None]), 0.0)
    dP = dO @ V.T                                         # [q, k]
    if emulate is not None:
        c = _f32(_f32(ms) + _f32(logl))
        Pb = np.where(adm, np.exp(t - c[:, None]), 0.0)
        dP = _f32(dP)
    delta = (Pb * dP).sum(1)
    if emulate is not None:
        delta = _f32(delta)
    dl = np.roll(delta, 1) if mut == "delta_shifted" else delta
    dS = Pb * (dP - dl[:, None])
    P16, dS16 = Pb, dS
    if emulate is not None:
        P16, dS16 = round_to(Pb, emulate), round_to(dS, emulate)
    if mut == "p_rounded_bf16":
        P16 = round_to(Pb, BF)
    dSq, dSk = dS16, dS16
    if mut == "drop_block":      # key block 0 missing from the query owner's sums, query block 1 from the key owner's
        P16, dSq, dSk = P16.copy(), dS16.copy(), dS16.copy()
        dSq[:, :BLK] = 0.0
        dSk[BLK:2 * BLK] = 0.0
        P16[BLK:2 * BLK] = 0.0
    dV, dQ, dK = P16.T @ dO, scale * (dSq @ K), scale * (dSk.T @ Q)
    if mut == "kq_swapped":
        dK, dQ = dQ, dK
    r = dict(out=out, lse0=lse0, lse1=lse1, delta=delta, dV=dV, dK=dK, dQ=dQ)
    if emulate is not None:
        for k in ("out", "dV", "dK", "dQ"):
            r[k] = round_to(r[k], emulate)
        r["lse0"], r["lse1"] = np.where(has, _f32(ms), -np.inf), np.where(has, _f32(logl), -np.inf)
    if dtype is None or mut is not None or emulate is not None:
        return r

    # ---- the bound. Every term is a unit roundoff times the fp64 sum of absolute values of what is summed; the counts are read off
    # csrc/attention_causal.hip and named where they enter. Relative errors are in natural-log units of the exponent.
    u, uT, eta, eta32 = U32, UT[dtype], ETA[dtype], ETA[BF]
    A = adm.astype(np.float64)
    aQ, aK, aV, adO = np.abs(Q), np.abs(K), np.abs(V), np.abs(dO)
    nb = (np.arange(S) // BLK + 1).astype(np.float64)       # key blocks a query's row walks: kb = 0 .. qb
    # x: dh products accumulated in fp32 by dh / 16 chained MFMAs (`x = mfma32(K rows, qf[s], x)`, s < KS), any order: dh u sum|Q||K|,
    # doubled because MFMA accumulation need not round every addition the IEEE way (as gemm_bound, wgrad_bound)
    ex = 2.0 * dh * u * (aQ @ aK.T) * A
    tabs = np.where(adm, np.abs(t_all), 0.0)
    et = scale * ex + u * tabs                              # t = x * a.scale: one rounding
    d = np.where(adm, t - ms[:, None], 0.0)
    # forward exponential `exp2f((x[i] - mu) * L2E)`: the subtraction u |t - mu|, fl(log2 e) and the product 2 u |t - mu|, with
    # |t - mu| <= |d| (mu <= m, t <= mu); then every later block's alpha = exp2f((m - mu) * L2E) the same three roundings on its own
    # argument, and those arguments telescope to m_final - mu <= |d|: 6 u |d| in all
    e_arg = 6.0 * u * np.abs(d)
    # one rescale per key block (`l = l * alpha + ps`, `o[dt] *= alpha`): alpha's v_exp, the product and the sum
    resc = nb * (EPS_EXP + 2.0 * u)
    # l: 16 in-lane additions and the merge of the two lane halves (`ps += __shfl_xor(ps, 32)`) per block, on top of the rescale:
    # 19 roundings per block on a sum of non-negative terms; the terms' own errors enter as their P-weighted mean (et: as its maximum —
    # lse is shift invariant, so a perturbation of the logits moves it by at most the largest one); v_exp results flushed below 2^-126
    rel_l = et.max(1) + (P * e_arg).sum(1) + resc + EPS_EXP + 19.0 * nb * u + SP * eta32
    # lse0 + lse1 = m + logf(l): m is one of the fp32 logits as it stands, logf 1 ulp and the rounding of its result
    b_lse = rel_l + (EPS_LOG + 2.0 * u) * np.abs(logl)
    # P in the forward = e / l: the term, its rescales, l, `inv = 1.f / l` and `acc * mul` in store_t
    rho_f = et + e_arg + resc[:, None] + EPS_EXP + rel_l[:, None] + 3.0 * u
    # e rounded to T by pack_acc before it is the MFMA's B operand (fp16: the subnormal step, in units of the running maximum's
    # e = 1, which every later alpha <= 1 and 1 / l <= 1 only shrink)
    wP = (P * (rho_f + uT * (1.0 + rho_f)) + eta / ls[:, None]) * A
    acc = 2.0 * SP * u                                      # 32 ceil(S / 32) terms accumulated by the MFMAs (rows beyond S are zeros)
    fin = lambda b, ref: b * (1.0 + uT) + uT * np.abs(ref) + eta  # noqa: E731  (f32_to_bits<T> in store_t)
    b_out = fin(wP @ aV + acc * (P @ aV), out)
    # backward exponential `exp2f((p[i] * a.scale - c) * L2E)`, c = fl(lse0 + lse1) of the forward's own planes: the logit as above,
    # the forward's lse error, the addition u |c|, the subtraction and the product with fl(log2 e) 3 u |t - c|
    cabs = np.abs(ms + logl)
    lp = np.where(adm, np.abs(t - (ms + logl)[:, None]), 0.0)
    rho_b = (et + b_lse[:, None] + u * cabs[:, None] + 3.0 * u * lp + EPS_EXP) * A
    absdP = np.abs(dP)
    e_dp = 2.0 * dh * u * (adO @ aV.T)                      # dP: dh / 16 chained MFMAs (`dp = mfma32(V rows, gf[s], dp)`)
    # delta: `dsum = fmaf(p[i], dp[i], dsum)` over the 16 registers of every key block, then the two lane halves added: 16 nb + 1
    # sequential roundings on sum |P dP|, plus the terms' own errors (a P flushed below 2^-126 loses at most that)
    b_delta = (P * absdP * rho_b + P * e_dp + eta32 * absdP * A).sum(1) + (16.0 * nb + 1.0) * u * (P * absdP).sum(1)
    G = (dP - delta[:, None]) * A
    # dS = p (dp - delta): the subtraction and the product (`p[i] *= dp[i] - delta`; key owner: `pv * (dp[i] - sd[j])`, the delta read
    # back from memory as the query owner stored it)
    e_ds = P * (np.abs(G) * (rho_b + 2.0 * u) + e_dp + b_delta[:, None]) + eta32 * np.abs(G)
    w_ds = (e_ds + uT * (np.abs(dS) + e_ds) + eta) * A      # dS rounded to T by pack_acc
    wPb = (P * (rho_b + uT * (1.0 + rho_b)) + eta) * A      # P rounded to T by pack_acc
    aS = np.abs(dS)
    r.update(b_out=b_out, b_lse=b_lse, b_delta=b_delta, b_dV=fin(wPb.T @ adO + acc * (P.T @ adO), dV),
             b_dQ=fin(scale * (w_ds @ aK + (acc + u) * (aS @ aK)), dQ),       # (+ u: `acc * mul` with mul = a.scale in store_t)
             b_dK=fin(scale * (w_ds.T @ aQ + (acc + u) * (aS.T @ aQ)), dK))
    return r


def causal_ref(Q, K, V, valid, dO, dtype=None, mut=None, emulate=None):
    """Q, K, V, dO fp64 [B, S, H, dh], valid bool [B, S] -> the results and bounds of head_ref stacked: out / dQ / dK / dV (and
    their b_) [B, S, H, dh], lse0 / lse1 / delta (b_lse, b_delta) [B, H, S], lse = lse0 + lse1 (-inf on a row without keys)"""
    B, S, H, dh = Q.shape
    heads = [[head_ref(Q[b, :, h], K[b, :, h], V[b, :, h], valid[b], dO[b, :, h], dh, dtype, mut, emulate) for h in range(H)]
             for b in range(B)]
    r = {}
    for k in heads[0][0]:
        a = np.array([[heads[b][h][k] for h in range(H)] for b in range(B)])   # [B, H, S(, dh)]
        r[k] = a.transpose(0, 2, 1, 3) if a.ndim == 4 else a
    r["lse"] = r["lse0"] + r["lse1"]
    return r


def violations(r, got, name):
    """bool array: the elements of got[name] outside the bound of r[name]. lse on a row without keys has to BE -inf; a NaN is
    outside every bound."""
    ref, g = r[name], got[name]
    bad = ~(np.abs(g - np.where(np.isfinite(ref), ref, 0.0)) <= r["b_" + name])
    if name == "lse":
        bad = np.where(np.isfinite(ref), bad, ~(g == ref))
    return bad


def ratios(r, got, name):
    """error / bound per element (0 where the reference is -inf: those are compared exactly)"""
    ref = r[name]
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        return np.where(fin, np.abs(got[name] - np.where(fin, ref, 0.0)) / np.maximum(r["b_" + name], 1e-300), 0.0)


# ------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """One forward + backward call: the shape, the layout and the key masks of its batch elements."""
    id: str
    B: int
    S: int
    H: int
    dh: int
    layout: str = "plain"   # plain: ld_qkv = ld_dqkv = 3 D, sections K | Q | V at (0, D, 2 D), ld_out = ld_dout = D. wide: ld_qkv = ld_dqkv =
    #                         3 D + 8, ld_out = D + 8, ld_dout = D + 16, the pad columns of qkv and dout NaN. perm: plain with q_off = 0,
    #                         v_off = D, k_off = 2 D
    masks: tuple = ("full",)  # per batch element, cycled: full | prefix (the decoder's: keys 0 .. n - 1, n mid-block) | hole (a run in the
    #                           middle and every fifth key) | key0 (key 0 masked: query 0 has no key) | block (one whole 32-key block
    #                           masked; the only block at S <= 32: no query has a key)

    @property
    def D(self):
        return self.H * self.dh

    @property
    def NB(self):
        return cdiv(self.S, BLK)

    @property
    def offs(self):
        """k_off, q_off, v_off"""
        D = self.D
        return (2 * D, 0, D) if self.layout == "perm" else (0, D, 2 * D)

    @property
    def lds(self):
        """ld_qkv (= ld_dqkv), ld_out, ld_dout"""
        D = self.D
        return (3 * D + 8, D + 8, D + 16) if self.layout == "wide" else (3 * D, D, D)

    @property
    def s_class(self):
        S = self.S
        return ("one row" if S == 1 else "ragged single block" if S < BLK else "exact blocks" if S % BLK == 0
                else "blocks plus one row" if S % BLK == 1 and S < 3 * BLK else "many blocks ending ragged")

    def valid(self):
        """bool [B, S]: the key masks"""
        S, NB = self.S, self.NB
        v = np.ones((self.B, S), dtype=bool)
        for b in range(self.B):
            kind = self.masks[b % len(self.masks)]
            if kind == "prefix":
                n = max(1, S - 13 if (S - 13) % BLK else S - 14)
                v[b, n:] = False
            elif kind == "hole":
                v[b, 3::5] = False
                v[b, S // 2:S // 2 + 9] = False
            elif kind == "key0":
                v[b, 0] = False
            elif kind == "block":
                kb = (NB - 1) // 2
                v[b, BLK * kb:BLK * (kb + 1)] = False
            else:
                assert kind == "full", kind
        return v


MASK_KINDS = ("full", "prefix", "hole", "key0", "block")
S_CLASSES = ("one row", "ragged single block", "exact blocks", "blocks plus one row", "many blocks ending ragged")


def _cases():
    """every S at every head size; the heads 1 | 2 | 8 and the three layouts rotated over the head sizes so that each head size meets
    both non-contiguous layouts and every mask kind, B H <= 24 everywhere, the largest case B = 2, H = 2, S = 257"""
    rows = (  # S, B, (H per head size 16 / 32 / 64), (layout per head size), masks
        (1, 3, (2, 8, 1), ("plain", "wide", "perm"), ("full", "key0", "full")),
        (31, 2, (8, 1, 2), ("wide", "perm", "plain"), ("prefix", "hole")),
        (32, 3, (1, 2, 8), ("perm", "plain", "wide"), ("full", "key0", "block")),
        (33, 2, (2, 8, 1), ("wide", "perm", "plain"), ("key0", "prefix")),
        (64, 2, (2, 1, 2), ("plain", "wide", "perm"), ("block", "hole")),
        (65, 3, (1, 2, 8), ("perm", "plain", "wide"), ("full", "block", "key0")),
        (97, 2, (8, 2, 1), ("plain", "wide", "perm"), ("hole", "block")),
        (257, 2, (2, 2, 2), ("wide", "perm", "wide"), ("prefix", "block")),
    )
    out = []
    for S, B, Hs, layouts, masks in rows:
        for dh, H, layout in zip((16, 32, 64), Hs, layouts):
            out.append(Case(f"d{dh}-s{S}-b{B}h{H}-{layout}", B, S, H, dh, layout, masks))
    return tuple(out)


CASES = _cases()
CASE = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------ operands
LATE_STEP = 24.0    # natural-log units a logit gains per 32-key block (late): 20 ln 2 = 13.9 and some ten for the unit-scale columns
# ... and loses (early): e^-17.4 = 2^-25 is half of fp16's smallest subnormal, e^-92.9 = 2^-134 half of bf16's (it has fp32's exponent
# range), again with some ten in hand for the spread of the logits inside a block. test_causal_refs_cpu.py checks both on the operands
EARLY_STEP = {FP: 28.0, BF: 112.0}
Q0 = 8.0            # Q[q, 0] in the late and early modes: K[k, 0] = +- g (k // 32) with scale Q0 g >= the step


def step_of(dh, dtype, mode):
    """(g, the logit step per block it gives) of a late / early case"""
    want = LATE_STEP if mode == "late" else EARLY_STEP[dtype]
    g = math.ceil(want / (scale_of(dh) * Q0))
    return g, scale_of(dh) * Q0 * g


def _seed(c, dtype, mode):
    return [CASES.index(c), DTYPES.index(dtype), MODES.index(mode), 20263]


@functools.lru_cache(maxsize=None)
def operands(cid, dtype, mode):
    """The case's operands as CPU tensors, deterministic (shared by the tests: leave them unchanged): qkv [B S, ld_qkv], dout
    [B S, ld_dout], keymask uint8 [B, S]. Pad columns hold NaN: the kernels must never read them.
    real: unit-scale normal Q, K, V, dO.
    late: Q[q, 0] = 8 and K[k, 0] = g (k // 32): every block's logits lie a step of at least 24 above the block's before, so each
    row's maximum arrives in its last admissible block and everything gathered before is rescaled by alpha < 2^-20.
    early: K[k, 0] = -g (k // 32): the maximum sits in the first admissible block and every later e = exp(t - m) is below half the
    activation type's smallest positive number (the step: EARLY_STEP), so it is rounded to exactly 0.
    The other columns are unit-scale normals in both, so the logits inside a block differ as in `real`."""
    c = CASE[cid]
    rng = np.random.default_rng(_seed(c, dtype, mode))
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    ldq, ldo, lddo = c.lds
    Q, K, V, dO = (rng.standard_normal((B, S, H, dh)) for _ in range(4))
    if mode != "real":
        g, _ = step_of(dh, dtype, mode)
        Q[..., 0] = Q0
        K[..., 0] = (g if mode == "late" else -g) * (np.arange(S) // BLK)[None, :, None]

    def padded(a, ld):
        full = torch.full((a.shape[0], ld), float("nan"), dtype=dtype)
        full[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dtype)
        return full

    qkv = np.zeros((B * S, 3 * D))
    for a, off in zip((K, Q, V), c.offs):
        qkv[:, off:off + D] = a.reshape(B * S, D)
    return dict(qkv=padded(qkv, ldq), dout=padded(dO.reshape(B * S, D), lddo), keymask=torch.from_numpy(c.valid().astype(np.uint8)))


def sections(c, qkv, dout):
    """Q, K, V, dO fp64 [B, S, H, dh] out of the (16-bit) qkv and dout tensors of a case"""
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    q, d = qkv.double().numpy(), dout.double().numpy()
    K, Q, V = (q[:, off:off + D].reshape(B, S, H, dh) for off in c.offs)
    return Q, K, V, d[:, :D].reshape(B, S, H, dh)


@functools.lru_cache(maxsize=None)
def references(cid, dtype, mode):
    """results and bounds of a case (computed once, shared: leave unchanged)"""
    c, o = CASE[cid], operands(cid, dtype, mode)
    Q, K, V, dO = sections(c, o["qkv"], o["dout"])
    return causal_ref(Q, K, V, c.valid(), dO, dtype)


def variant(cid, dtype, mode, **kw):
    """causal_ref of the case's operands with mut= or emulate="""
    c, o = CASE[cid], operands(cid, dtype, mode)
    Q, K, V, dO = sections(c, o["qkv"], o["dout"])
    return causal_ref(Q, K, V, c.valid(), dO, **kw)
