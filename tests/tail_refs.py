"""A plain fp64 reference of the one-launch position-0 tails of the top encoder layer (csrc/row_tail.hip: mst_row_tail_fwd, _fwd_ride,
_fwd_ride_shadows, mst_row_tail_bwd, _bwd_ride), the bounds they are held to and the table of cases; no GPU, no library. Built on
tests/rowblock_refs.py: the stage classes, the fp64 stages, the derived bounds, the hard rows and the keep decision are imported
from there, not restated; this module adds the tails' two chains (plan), their layout, their riders and the launch's decisions.

STAGE-WISE, as there: every stored tensor is held to an fp64 evaluation of its own stage on what the DEVICE stored for the stage
above. The chains (include/mst_hip.h; dropout counter = r * phys_stride * N + column at sites site0, site0 + 1, site0 + 2):
  forward    Gemm   h1 = att Wp^T + bp, dropout, + resid                       LnFwd  h1 -> x1, mean1, rstd1
             Gemm   a = relu(x1 W1^T + b1), dropout                            Gemm   h2 = a W2^T + b2, dropout, + x1
             LnFwd  h2 -> x2, mean2, rstd2
  backward   LnBwd  (dy, h2, mean2, rstd2, g2), mask mode 1, site0 + 2 -> dh, dhm, dg2 / db2 +=
             Gemm   dpre = dhm W2t^T, gate a, alpha 1 / (1 - p)                Gemm   dx1 = dpre W1t^T + dh
             LnBwd  (dx1, h1, mean1, rstd1, g1), mask mode 1, site0 -> dh1, dh1m, dg1 / db1 +=
             Gemm   datt = dh1m Wpt^T
At p = 0 the kernel still stores dhm and dh1m: they are checked as copies of dh / dh1 (the mask is all ones).
(alpha: the kernel multiplies by the forward's keep scale 65536 / (65536 - floor(65536 p)), the header says 1 / (1 - p): 1.1e-5 apart
at p = 0.2, a third of the fp32 term 2 (K + 16) u S of the bound at K = 256, so either reference holds a correct kernel.)

BOUNDS: rowblock_refs' derived ones, unchanged. gemm_bound's factor 2 covers the four K quarters that meet in LDS (quarter_sum: four
partial MFMA sums, three more additions); the dgamma / dbeta bound covers 4 rows per lane, then 16 waves through LDS, then one
atomic onto the initial value (M + 1 terms in another order: 2 (M + 16) u of the sum of magnitudes). No term had to be added
after the MI355X run (docs/kernel_notes.md has the measured ratios).

LAYOUT of every case. Row r of a 2-D buffer sits at physical row r * (the buffer's own stride); every other physical row, every pad
column (8 behind each row: weights get ld = K + 8) and the guard rows hold NaN on inputs and SENTINEL on outputs:
  forward    att 2, resid 3, h1 / x1 / h2 / x2 (rs_d) 4, a 2 (width F)        backward   dy 2, h2 / h1 (rs_d) 4, a 2,
  dh / dhm / dx1 / dh1m (rs_c) 1, dpre 1, dh1 3, datt 5  -> rs_dy, rs_a, rs_c, rs_dpre, rs_dh1, rs_datt pairwise different
  statistics at index 3 r (stat_stride) while the dropout counter's row is 5 r (phys_stride); dgamma / dbeta start at INIT;
  dropout_seed = SEED and the seed word behind dropout_seed_ptr = SEED_WORD, both non-zero.
Operands: rowblock_refs.hard_rows (offset rows, a constant row, a spike row; the second LayerNorm's constant and spike rows 8 rows
further down; for B < 15 the hard rows that fit), a zero gamma, `a` of the backward cases a ReLU output with exact zeros, the
backward cases' statistics the fp32-rounded fp64 statistics of h1 / h2. In the forward cases h1 and h2 are computed: the hard
rows are in resid (and att's constant row is zero, so that h1's stays near constant: resid + dropout(bp))."""
import os
import sys
import zlib
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowblock_refs as R  # noqa: E402
from rowblock_refs import (BF, FP, DTYPES, DT_NAME, SENTINEL, PAD, GUARD, INIT, NAN, SEED, SEED_WORD, P_DROP, EPS,  # noqa: E402,F401
                           Buf, Gemm, LnFwd, LnBwd, gemm_ref, gemm_bound, ln_fwd_ref, ln_bwd_ref, keep_scale, hard_rows, _gamma,
                           check, intact, describe, outputs, gather, scatter, owned, plan, Result,
                           OFFSET_ROW, CONST_ROW, SPIKE_ROW, ZERO_GAMMA, LEAD_SHIFT)

SITE0 = 6
PHYS_STRIDE, STAT_STRIDE = 5, 3
STRIDES = dict(att=2, resid=3, d=4, a=2, dy=2, c=1, dpre=1, dh1=3, datt=5)   # physical rows per logical row, per buffer family
# riders: (samples, rows per sample T: rows 1..T of every T + 1, N, K)
RIDERS = {"one": (1, 128, 128, 64),      # one 128 x 128 tile
          "many": (15, 128, 1920, 64),   # 225 tiles of 128 rows (M % 256 != 0): more than one round of riding workgroups
          "big": (7, 256, 2048, 64)}     # 224 tiles of 128 rows > 208, M and T multiples of 256: 112 tiles of 256 rows
SHADOW_SHAPES = ((10, 32), (293, 128), (256, 1024))   # three matrices, ragged ones included


@dataclass(frozen=True)
class Case:
    kind: str              # tail_fwd | tail_bwd | tail_chain (forward, then backward on what the forward launch stored)
    dtype: torch.dtype
    M: int                 # B: the position-0 rows
    D: int
    p: float = P_DROP
    rider: str = "none"    # none | one | many | big
    shadows: bool = False  # forward: the shadow refresh behind the rider's tiles

    @property
    def F(self):
        return 4 * self.D

    @property
    def groups(self):      # the dropout counter's row: r * phys_stride
        return (1, PHYS_STRIDE, 0)

    @property
    def id(self):
        return (f"{self.kind}-{DT_NAME[self.dtype]}-B{self.M}-D{self.D}-p{self.p:g}" + (f"-{self.rider}" if self.rider != "none" else "")
                + ("-shadows" if self.shadows else ""))


def _cases():
    out = []
    for dt in DTYPES:
        def C(kind, M, D, p=P_DROP, rider="none", shadows=False):
            out.append(Case(kind, dt, M, D, p, rider, shadows))
        # every B in each direction; both widths see 1, 17 and 64; every (width, rider tile height) kernel in each direction
        C("tail_fwd", 1, 128), C("tail_fwd", 15, 128, rider="many"), C("tail_fwd", 16, 128, p=0.0)
        C("tail_fwd", 17, 128, p=0.0, rider="one", shadows=True), C("tail_fwd", 64, 128, rider="big")
        C("tail_fwd", 1, 256, rider="one"), C("tail_fwd", 17, 256, rider="big", shadows=True), C("tail_fwd", 49, 256)
        C("tail_fwd", 64, 256, p=0.0, rider="many")
        C("tail_bwd", 1, 128, rider="one"), C("tail_bwd", 16, 128), C("tail_bwd", 17, 128, p=0.0, rider="big")
        C("tail_bwd", 49, 128, p=0.0), C("tail_bwd", 64, 128, rider="many")
        C("tail_bwd", 1, 256), C("tail_bwd", 15, 256, rider="one"), C("tail_bwd", 17, 256, p=0.0, rider="many")
        C("tail_bwd", 64, 256, rider="big")
        C("tail_chain", 49, 128), C("tail_chain", 64, 256)
    return tuple(out)


CASES = _cases()
# launched a second time, with other operands, into the same output buffers: one per direction and width
STALE = tuple(c.id for c in CASES if c.dtype == BF and (c.kind, c.M, c.D) in (("tail_fwd", 17, 128), ("tail_fwd", 49, 256), ("tail_bwd", 16, 128),
                                                                            ("tail_bwd", 15, 256)))


# ------------------------------------------------------------------------------------------ the chains
def _plan(c):
    D, F = c.D, c.F
    b, st = {}, []
    fwd, bwd = c.kind in ("tail_fwd", "tail_chain"), c.kind in ("tail_bwd", "tail_chain")

    def act(name, width, out, fam):
        b[name] = Buf("phys", width, out, stride=STRIDES[fam])

    def stat(name, out):
        b[name] = Buf("stat", 0, out, stride=STAT_STRIDE)

    def vec(name, width, out=False):
        b[name] = Buf("vec", width, out)

    def w(name, n, k):
        b[name] = Buf("w", k, False, n)

    if fwd:
        act("att", D, False, "att"), act("resid", D, False, "resid")
        w("Wp", D, D), vec("bp", D), vec("g1", D), vec("be1", D), w("W1", F, D), vec("b1", F), w("W2", D, F), vec("b2", D), vec("g2", D), vec("be2", D)
        for n in ("h1", "x1", "h2", "x2"):
            act(n, D, True, "d")
        act("a", F, True, "a")
        for n in ("mean1", "rstd1", "mean2", "rstd2"):
            stat(n, True)
        st += [Gemm("h1", "att", "Wp", D, bias="bp", p=c.p, site=SITE0, resid="resid"), LnFwd("h1", "g1", "be1", "x1", "mean1", "rstd1"),
               Gemm("a", "x1", "W1", D, bias="b1", relu=True, p=c.p, site=SITE0 + 1),
               Gemm("h2", "a", "W2", F, bias="b2", p=c.p, site=SITE0 + 2, resid="x1"), LnFwd("h2", "g2", "be2", "x2", "mean2", "rstd2")]
    if bwd:
        act("dy", D, False, "dy")
        if not fwd:
            act("h2", D, False, "d"), act("h1", D, False, "d"), act("a", F, False, "a"), vec("g1", D), vec("g2", D)
            for n in ("mean1", "rstd1", "mean2", "rstd2"):
                stat(n, False)
        w("W2t", F, D), w("W1t", D, F), w("Wpt", D, D)
        for n in ("dh", "dhm", "dx1", "dh1m"):
            act(n, D, True, "c")
        act("dpre", F, True, "dpre"), act("dh1", D, True, "dh1"), act("datt", D, True, "datt")
        for n in ("dg1", "db1", "dg2", "db2"):
            vec(n, D, True)
        inv = 1.0 / (1.0 - c.p)
        st += [LnBwd("dy", "h2", "mean2", "rstd2", "g2", "dh", "dhm", 1, c.p, SITE0 + 2, "dg2", "db2"),
               Gemm("dpre", "dhm", "W2t", D, alpha=inv, gate="a"), Gemm("dx1", "dpre", "W1t", F, resid="dh"),
               LnBwd("dx1", "h1", "mean1", "rstd1", "g1", "dh1", "dh1m", 1, c.p, SITE0, "dg1", "db1"), Gemm("datt", "dh1m", "Wpt", D)]
    return b, st


for _k in ("tail_fwd", "tail_bwd", "tail_chain"):
    R.PLANS[_k] = _plan

WEIGHT_SCALE = dict(Wp=0.06, W1=0.06, W2=0.03, W2t=0.05, W1t=0.05, Wpt=0.06)


def _gen(c, what, salt):
    return torch.Generator().manual_seed(zlib.crc32(f"{c.id}/{what}/{salt}".encode()))


def operands(c, salt=0):
    """the case's inputs as CPU tensors, seeded (salt: another draw of the same case), 16-bit-rounded; pad columns and every row that
    is not a position-0 row hold NaN"""
    bufs, _ = plan(c)
    g = _gen(c, "operands", salt)
    o = {}
    for name, s in bufs.items():
        if s.out or s.rows == "stat":
            continue
        t = R._alloc(c, s, NAN)
        if s.rows == "phys":
            if name == "a":        # the forward's hidden activation: ReLU and dropout leave about 60 % exact zeros
                v = torch.randn((c.M, s.width), generator=g).double().numpy()
                v = R._r16(np.where(v > 0.25, v, 0.0), c.dtype)
            elif name == "dy":
                v = R._r16(torch.randn((c.M, s.width), generator=g).double().numpy() * 0.5, c.dtype)
            else:
                v = hard_rows(g, c.M, s.width, c.dtype, shift=LEAD_SHIFT if name == "h1" else 0)
                if name == "att":
                    v *= 0.5
                    if c.M > CONST_ROW:
                        v[CONST_ROW] = 0.0
            scatter(c, s, t, v)
        elif s.rows == "w":
            t[:, :s.width] = (torch.randn((s.n, s.width), generator=g) * WEIGHT_SCALE[name]).to(c.dtype)
        else:
            if name in ("g1", "g2"):
                t[:] = torch.from_numpy(_gamma(g, s.width))
            else:
                t[:] = torch.randn((s.width,), generator=g) * (0.5 if name in ("be1", "be2") else 0.1)
        o[name] = t
    for mean, rstd, x in (("mean1", "rstd1", "h1"), ("mean2", "rstd2", "h2")):
        if not bufs[mean].out:
            xs = gather(c, bufs[x], o[x])
            mu = xs.mean(1)
            var = ((xs - mu[:, None]) ** 2).mean(1)
            for name, v in ((mean, mu), (rstd, 1.0 / np.sqrt(var + EPS))):
                t = R._alloc(c, bufs[name], NAN)
                scatter(c, bufs[name], t, v)
                o[name] = t
    o["seed_word"] = torch.tensor([SEED_WORD - (1 << 64)], dtype=torch.int64)
    return o


def strides(c):
    """the element row strides the launch is handed, from the buffers' shapes: name -> (physical rows per row) * (width + PAD)"""
    bufs, _ = plan(c)
    return {n: s.stride * (s.width + PAD) for n, s in bufs.items() if s.rows == "phys"}


# ------------------------------------------------------------------------------------------ riders and shadows
def rider_operands(c, backward):
    """the riding GEMM of a case: rows 1..T of every T + 1 on A and C (row 0 of every sample: NaN in A, SENTINEL in C), bias on the
    forward rider, a residual on C's physical rows on the backward rider. -> dict(A, W, bias | resid, C, M, N, K, T)"""
    Bg, T, N, K = RIDERS[c.rider]
    g = _gen(c, "rider", int(backward))
    Md = Bg * (T + 1)
    own = (np.arange(Md) % (T + 1)) != 0
    A = torch.full((Md, K + PAD), NAN, dtype=c.dtype)
    A[torch.from_numpy(own), :K] = torch.randn((Bg * T, K), generator=g).to(c.dtype)
    W = torch.full((N, K + PAD), NAN, dtype=c.dtype)
    W[:, :K] = (torch.randn((N, K), generator=g) * 0.08).to(c.dtype)
    Cm = torch.full((Md + GUARD, N + PAD), SENTINEL, dtype=c.dtype)
    o = dict(A=A, W=W, C=Cm, M=Bg * T, N=N, K=K, T=T, own=own)
    if backward:
        r = torch.full((Md, N + PAD), NAN, dtype=c.dtype)
        r[torch.from_numpy(own), :N] = torch.randn((Bg * T, N), generator=g).to(c.dtype)
        o["resid"] = r
    else:
        o["bias"] = torch.randn((N,), generator=g) * 0.1
    return o


def rider_check(c, r, C_got):
    """the riding GEMM against fp64 (rowblock_refs.gemm_bound = gemm_refs' bound) -> (Result, complaints about rows and columns it
    must leave alone)"""
    N, K, own = r["N"], r["K"], r["own"]
    A, W = r["A"].double().numpy()[own, :K], r["W"].double().numpy()[:, :K]
    bias = r["bias"].double().numpy() if "bias" in r else None
    resid = r["resid"].double().numpy()[own, :N] if "resid" in r else None
    ref, S = gemm_ref(A, W, bias, 1.0, False, None, False, resid, None)
    got = C_got.double().numpy()
    res = Result("rider C", "gemm A x W", got[:len(own)][own, :N], ref, gemm_bound(c.dtype, K, ref, S))
    mask = np.zeros(got.shape, dtype=bool)
    mask[:len(own)][own, :N] = True
    bad = []
    if not (got[~mask] == SENTINEL).all():
        bad.append(f"rider C: {int((got[~mask] != SENTINEL).sum())} elements outside the output were written (row 0 of a sample, pad columns, guard rows)")
    return res, bad


def shadow_operands(c):
    """mst_transpose_shadows' list for SHADOW_SHAPES -> dict(w fp32 flat, wt16 (filled with 9), desc, prefix, n_mat, tiles, views)"""
    g = _gen(c, "shadows", 0)
    desc, prefix, so, do, views = [], [0], 0, 0, []
    for rr, cc in SHADOW_SHAPES:
        ldt = (rr + 7) // 8 * 8
        desc += [so, do, rr, cc]
        views.append((so, do, rr, cc, ldt))
        so, do = so + rr * cc, do + cc * ldt
        prefix.append(prefix[-1] + ((rr + 31) // 32) * ((cc + 31) // 32))
    return dict(w=torch.randn((so,), generator=g), wt16=torch.full((do + 64,), 9.0, dtype=c.dtype), desc=torch.tensor(desc, dtype=torch.int64),
                prefix=torch.tensor(prefix, dtype=torch.int64), n_mat=len(SHADOW_SHAPES), tiles=prefix[-1], views=views, end=do)


def shadow_check(c, sh, wt16_got):
    """exact transposes with zeroed pad columns, nothing written behind the last matrix -> complaints"""
    bad = []
    for k, (so, do, rr, cc, ldt) in enumerate(sh["views"]):
        got = wt16_got[do:do + cc * ldt].view(cc, ldt)
        want = sh["w"][so:so + rr * cc].view(rr, cc).t().to(c.dtype)
        if not torch.equal(got[:, :rr], want):
            bad.append(f"shadow {k} ({rr} x {cc}): {int((got[:, :rr] != want).sum())} elements are not the rounded transpose")
        if not (got[:, rr:] == 0).all():
            bad.append(f"shadow {k} ({rr} x {cc}): pad columns not zeroed")
    if not (wt16_got[sh["end"]:] == 9.0).all():
        bad.append("shadows: written behind the last matrix")
    return bad


# ------------------------------------------------------------------------------------------ the launch's decisions, restated
def ride_form(backward, D, rider=None, sh_tiles=0):
    """mst_row_tail_form's six entries restated from csrc/row_tail.hip (ride_shape, ride_grid): rider (M, N, T) or None
    -> dict(kernel, ride_rows, tiles, grid, lds, tickets)"""
    G = D // 16
    f = dict(kernel=0 if D == 256 else 1, ride_rows=0, tiles=0, grid=12 * G, lds=0, tickets=0)
    if rider is not None:
        M, N, T = rider
        t128 = (M // 128) * (N // 128)
        big = t128 > 7 * 32 - 16 and M % 256 == 0 and (T <= 0 or T % 256 == 0)
        f["ride_rows"], f["tiles"] = (256, (M // 256) * (N // 128)) if big else (128, t128)
        f["lds"] = 2 * (256 + 128) * 64 * 2 if big else 128 * (128 + 4) * 4
        f["kernel"] += 4 if big else 2
        over = ((f["tiles"] * 8 + 6) // 7 + G - 1) // G + 1
        f["grid"] = G * min(max(over, 9), 16)
    if not backward:
        f["tickets"] = (sh_tiles + 15) // 16
        if f["tickets"]:
            f["lds"] = max(f["lds"], 16 * 32 * 33 * 4)
    else:
        f["lds"] = max(f["lds"], 2 * 64 * (D + 8) * 2 + 16 * 2 * D * 4 + 4 * 64 * 16 * 4 + 2 * D * 4)
    return f


def case_forms(c):
    """[(backward, form)] of the launches a case makes"""
    rid = None
    if c.rider != "none":
        Bg, T, N, _ = RIDERS[c.rider]
        rid = (Bg * T, N, T)
    sh = sum(((rr + 31) // 32) * ((cc + 31) // 32) for rr, cc in SHADOW_SHAPES) if c.shadows else 0
    out = []
    if c.kind in ("tail_fwd", "tail_chain"):
        out.append((0, ride_form(0, c.D, rid, sh)))
    if c.kind in ("tail_bwd", "tail_chain"):
        out.append((1, ride_form(1, c.D, rid, 0)))
    return out
