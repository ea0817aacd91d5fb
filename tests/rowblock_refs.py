"""A plain fp64 reference of the LayerNorm-fused row-block launches (no GPU, no library), the tolerances they are held to, and the
table of cases: gemm_epilogue_ln (mst_gemm_nt_ln mode 1 / 2), ffn_ln_body (mst_ffn_ln_fwd, mst_proj_ffn_ln_fwd, mst_ffn_ln_bwd,
mst_ffn_ln_bwd_lead, mst_dec_tail_step) and the stand-alone kernels of csrc/layernorm.hip.

STAGE-WISE. Every tensor a launch stores is a function of the launch's inputs and of tensors the same launch also stores, each
rounded to the activation type before the next stage reads it (include/mst_hip.h: "the value the unfused pipeline would have stored
and re-read"). A launch is therefore a list of stages (plan()), and check() holds each stored tensor to an fp64 evaluation of its
own stage whose inputs are what the DEVICE stored for the stage above (the launch's inputs where there is none). A stage's error is
one stage of fp32 arithmetic plus one store rounding, whatever the length of the chain, and a failure names the stage.

The stages, in the header's order (mst_gemm_args / mst_ln_args / mst_ln_bwd_in):
  gemm     t = alpha (A B^T + bias) -> ReLU -> u = dropout(t) [self_resid: u += t] -> + resid -> zero where gate <= 0
           (gemm_refs.gemm_ref's structure with its S, the same expression on absolute values)
  ln_fwd   mean, rstd = 1 / sqrt(var + eps) (biased variance, eps inside the root) of the 16-bit-rounded row h,
           y = (h - mean) rstd gamma + beta; mean and rstd at the PHYSICAL row
  ln_bwd   xh = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean(g) - xh mean(g xh)), dgamma += sum_m dy xh, dbeta += sum_m dy;
           mask mode 0: dx; 1: also dx keep / (1 - p); 2: dx (1 + keep / (1 - p)), dx 2 at p = 0. The keep decision
           (gemm_refs.keep_mask) is taken at counter (physical row) * N + column. Where dy is not stored (mst_gemm_nt_ln mode 2, the
           second half of mst_ffn_ln_bwd) the stage is ln_bwd(gemm(...)) and the GEMM's error is carried through dy -> dx.

BOUNDS, derived (u = 2^-24 the fp32 unit roundoff; u_out = 2^-8 bf16, 2^-11 fp16; a length-n fp32 sum in any order with the few
operations around it costs (n + 16) u times the sum of absolute values, twice that where MFMAs accumulate or an in-workgroup LDS
reduction reorders it; a 16-bit store costs u_out |ref| and carries the fp32 error E as E (1 + u_out); fp16 stores may land on a
subnormal: + 2^-25):
  gemm     gemm_refs.gemm_bound:  u_out |ref| + 2 (K + 16) u S (1 + u_out) + floor
  mean     fp32 only:  b_mean = (n + 16) u mean|h|
  rstd     fp32 only. The kernel forms d_i = fl(h_i - m') with m' = mean + delta, |delta| <= b_mean, then var' = fl(sum d_i^2 / n).
           sum (h_i - m')^2 / n = var + delta^2 EXACTLY (the cross term 2 delta sum(h_i - mean) vanishes: that is what the two-pass
           form buys, and why a one-pass E[x^2] - mean^2, whose error is (n + 16) u E[x^2], is refused on a row with mean^2 >> var),
           so the conditioning of the variance enters at second order only, as delta^2, which on a constant row (var = 0) is all
           there is beside eps. With the subtraction's, the squares' and the sum's roundings:
               |var' - var| <= delta^2 + (n + 20) u (var + delta^2),      and the addition of eps: + u (var + eps)
           rel_v = that / (var + eps);  b_rstd = rstd (rel_v / 2 + 4 u)   (root and division, correctly rounded, with slack)
  y        E_xh = rstd b_mean + |xh| (rel_v / 2 + 6 u);  E_y = |gamma| E_xh + 2 u (|xh gamma| + |beta|);  u_out |y| + E_y (1 + u_out)
  dx       c = (n + 32) u covers g's product, the two row sums, xh's error (3 u |xh|, scaled by |mean(g xh)| <= mean|g xh|) and the
           final three operations:
               E = rstd c (|g| + mean|g| + |xh| mean|g xh|)
           plus, where dy is not stored and carries the GEMM's error e (its whole gemm bound: the kernel rounds dy to 16 bits), the
           linear map dy -> dx on absolute values:  rstd (|gamma| e + mean(|gamma| e) + |xh| mean(|gamma| e |xh|)).
           mode 1's second output: k E (1 + 2 u); mode 2: (1 + k) E (1 + 2 u); then the store.
  dgamma   terms dy xh (16-bit-exact dy times fp32 xh: 4 u each for xh's error and the product), summed over M rows by 8 or 16 row
           groups of a workgroup, through LDS, then by atomics or partial rows:  2 (M + 16) u (sum|dy xh| + |initial|) + 4 u sum|dy xh|
           (+ sum e |xh| where dy carries e);  dbeta: 2 (M + 16) u (sum|dy| + |initial|) (+ sum e)
           The stand-alone kernel at M = 16389 needs no wider term: counted off layernorm_bwd_kernel, a column's M terms are added
           per wave in row order (5 at most there), then over the 16 waves of a workgroup through LDS, then over 256 workgroups by
           atomics or partial rows: every path is a sum of the same M terms in SOME order, which (M + 16) u already covers.
No constant above was chosen after looking at a GPU result.

The dropout keep decision is imported from gemm_refs (checked there against csrc/common.hpp), not restated.

Other reference modules build on this one (tests/tail_refs.py: the one-launch position-0 tails): they register the plan of their own
case kinds in PLANS, give a buffer a row stride of its own (Buf.stride) where a launch takes one per tensor, and share check(),
intact(), the stages and the bounds. None of that changes what the cases of this module compute."""
import os
import sys
import zlib
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_refs import BF, FP, DTYPES, DT_NAME, SENTINEL, keep_mask  # noqa: E402,F401

U = 2.0 ** -24
EPS = float(np.float32(1e-5))
SEED, SEED_WORD = 0x0123456789ABCDEF, 0xF00DFACE5EED1234
P_DROP = 0.2
PAD, GUARD = 8, 2          # pad columns behind every row, guard rows behind every output
INIT = 1.0                 # dgamma / dbeta are ACCUMULATED INTO: they start at this value
NAN = float("nan")
# dropout sites of the launches' GEMMs / LayerNorm masks (any distinct numbers)
SITE_PROJ, SITE_FF1, SITE_FF2, SITE_LEAD, SITE_LN = 3, 4, 5, 7, 2


def u_out(dtype):
    return 2.0 ** -8 if dtype == BF else 2.0 ** -11


def floor_(dtype):
    return 2.0 ** -25 if dtype == FP else 0.0


# ------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    kind: str              # ffn_fwd | ffn_bwd | gemm_ln_fwd | gemm_ln_bwd | ln | dec_tail
    dtype: torch.dtype
    M: int                 # logical rows
    D: int                 # row width (N of the LayerNorm)
    F: int = 0             # ffn: hidden width; gemm_ln: K
    groups: tuple = None   # (rows per group, stride, offset): ffn / dec_tail row groups, gemm_ln C remap; ln: (1, row_id_stride, 0)
    p: float = P_DROP
    resid: str = "none"    # none | x (the block's input) | other | self (self_resid)
    mode: int = 0          # LayerNorm-backward mask mode
    alpha: float = 1.0
    partials: bool = False
    proj: bool = False     # ffn_fwd: with the projection head
    lead: int = -1         # ffn_bwd: the leading LayerNorm backward's mask mode (-1: none)
    bias: bool = True
    tag: str = ""
    form: tuple = None     # ln: the instantiations the case is in the table for, (NV, R forward, R backward); asked of the library where it is run

    @property
    def id(self):
        g = "" if self.groups is None else "-g" + "_".join(map(str, self.groups))
        return (f"{self.kind}-{DT_NAME[self.dtype]}-M{self.M}-D{self.D}" + (f"-F{self.F}" if self.F else "") + g
                + (f"-{self.tag}" if self.tag else ""))


M_WHOLE, M_GUARDED = 1600, 1637    # 25 whole tiles: all four chunk rotations (blockIdx.x / 8) % 4; 26 tiles, the last ragged, grid % 8 != 0
RG = (64, 65, 1)                   # rows 1..T of every T + 1, T = 64
M_RG = 26 * 64                     # B = 26: 1664 logical rows, 1690 physical


# (M, D) -> (NV, R of the forward, R of the backward) the new stand-alone LayerNorm shapes are meant to reach
LN_FORMS = {(8197, 32): (1, 2, 2), (8197, 260): (2, 2, 1), (8197, 772): (4, 2, 1), (77, 512): (2, 1, 1), (1000, 512): (2, 1, 1),
            (1025, 128): (1, 1, 2), (1029, 128): (1, 1, 2), (1025, 256): (1, 1, 2), (1029, 256): (1, 1, 2), (16389, 32): (1, 2, 2),
            (8192, 32): (1, 1, 2), (8193, 32): (1, 2, 2)}


def _cases():
    out = []
    for dt in DTYPES:
        def C(kind, M, D, F=0, **kw):
            out.append(Case(kind, dt, M, D, F, **kw))
        # ---- ffn_ln forward: per (D, F) one whole-tile and one guarded case; between them resid = x, self_resid, p = 0, another residual
        fwd = {(128, 512): (dict(resid="x", tag="residx"), dict(resid="self", tag="self")),
               (128, 128): (dict(resid="other", tag="other"), dict(resid="x", p=0.0, tag="p0")),
               (256, 1024): (dict(resid="self", tag="self"), dict(resid="x", tag="residx")),
               (256, 512): (dict(resid="x", p=0.0, tag="p0"), dict(resid="other", tag="other"))}
        for (D, F), (kw_w, kw_g) in fwd.items():
            C("ffn_fwd", M_WHOLE, D, F, **kw_w)
            C("ffn_fwd", M_GUARDED, D, F, **kw_g)
        C("ffn_fwd", M_RG, 128, 512, groups=RG, resid="self", tag="rg")
        # ---- with the projection head
        for D, F in ((128, 512), (256, 1024)):
            C("ffn_fwd", M_WHOLE, D, F, proj=True, resid="x", tag="proj")
            C("ffn_fwd", M_GUARDED, D, F, proj=True, resid="self", tag="proj-self")
        C("ffn_fwd", M_RG, 128, 512, proj=True, groups=RG, resid="self", tag="proj-rg")
        # ---- ffn_ln backward: mask modes x residual x alpha x partials x whole / guarded
        bwd = {(128, 512): (dict(mode=1, resid="other", alpha=1.25, partials=True), dict(mode=2, alpha=1.25)),
               (128, 128): (dict(mode=0, resid="other", partials=True), dict(mode=1, alpha=1.25)),
               (256, 1024): (dict(mode=2, resid="other", alpha=1.25), dict(mode=1, resid="other", partials=True)),
               (256, 512): (dict(mode=1, partials=True), dict(mode=0, resid="other", alpha=1.25))}
        for (D, F), (kw_w, kw_g) in bwd.items():
            C("ffn_bwd", M_WHOLE, D, F, tag=f"m{kw_w['mode']}", **kw_w)
            C("ffn_bwd", M_GUARDED, D, F, tag=f"m{kw_g['mode']}", **kw_g)
        C("ffn_bwd", M_RG, 128, 512, groups=RG, mode=1, alpha=1.25, partials=True, tag="m1-rg")
        # ---- with the leading LayerNorm backward (the residual is its dx, as in the engine; lead mode 0: the first GEMM's operand
        # IS the residual, which the kernel then takes from its x tile)
        C("ffn_bwd", M_WHOLE, 128, 512, lead=1, mode=1, resid="x", alpha=1.25, partials=True, tag="lead1")
        C("ffn_bwd", M_GUARDED, 128, 512, lead=0, mode=0, resid="x", p=0.0, tag="lead0")
        C("ffn_bwd", M_WHOLE, 256, 1024, lead=0, mode=1, resid="x", partials=True, tag="lead0")
        C("ffn_bwd", M_GUARDED, 256, 1024, lead=1, mode=1, resid="x", alpha=1.25, tag="lead1")
        # ---- gemm_nt_ln: no remap, whole-tile groups (once-per-tile remap), ragged groups (per-row remap)
        G64, G50 = (64, 65, 1), (50, 53, 2)
        C("gemm_ln_fwd", 64, 128, 128, resid="other")
        C("gemm_ln_fwd", 200, 256, 1024, resid="other", groups=G50)
        C("gemm_ln_fwd", 1637, 128, 1024, resid="self", groups=G64, tag="self")
        C("gemm_ln_fwd", 1637, 256, 128, resid="other", groups=G50, p=0.0, tag="p0")
        C("gemm_ln_fwd", 200, 128, 128, resid="other", groups=G64)
        C("gemm_ln_fwd", 64, 256, 1024, resid="none", bias=False, tag="nobias")
        C("gemm_ln_fwd", 64, 256, 128, resid="other", groups=G64)
        C("gemm_ln_fwd", 64, 128, 1024, resid="other", groups=G50, alpha=1.7, tag="alpha")
        C("gemm_ln_fwd", 1637, 128, 128, resid="other")
        C("gemm_ln_bwd", 64, 128, 128, mode=0, resid="other", tag="m0")
        C("gemm_ln_bwd", 200, 256, 1024, mode=1, resid="other", groups=G50, tag="m1")
        C("gemm_ln_bwd", 1637, 128, 1024, mode=2, resid="other", groups=G50, partials=True, alpha=1.7, tag="m2")
        C("gemm_ln_bwd", 1637, 256, 128, mode=1, resid="other", groups=G64, partials=True, tag="m1")
        C("gemm_ln_bwd", 200, 128, 128, mode=2, groups=G64, tag="m2")
        C("gemm_ln_bwd", 200, 256, 128, mode=2, p=0.0, resid="other", tag="m2-p0")
        C("gemm_ln_bwd", 1637, 128, 128, mode=0, partials=True, tag="m0")
        C("gemm_ln_bwd", 64, 256, 1024, mode=0, resid="other", groups=G64, tag="m0")
        C("gemm_ln_bwd", 64, 128, 128, mode=1, resid="other", groups=G50, partials=True, tag="m1")
        C("gemm_ln_bwd", 1637, 256, 1024, mode=2, resid="other", tag="m2")
        # ---- the stand-alone kernels: forward, then backward on the statistics the forward stored
        for D, M, stride, mode, parts in ((32, 16, 1, 0, False), (40, 77, 4, 1, True), (128, 1000, 1, 2, True), (256, 77, 1, 1, False),
                                          (1024, 16, 4, 2, False), (1024, 1000, 1, 1, True), (40, 1000, 1, 0, False), (256, 1000, 4, 2, True),
                                          (128, 16, 1, 1, True), (32, 77, 1, 2, False)):
            C("ln", M, D, groups=(1, stride, 0), mode=mode, partials=parts, tag=f"m{mode}", form=(1 if D <= 256 else 4, 1, 1))
        C("ln", 77, 128, groups=(1, 1, 0), mode=2, p=0.0, tag="m2-p0", form=(1, 1, 1))
        # ---- ... in every instantiation <NV, R> (LN_FORMS below: what each shape is here for). Forward R = 2 from M = 8193
        # (2048 workgroups of 4 waves); backward R = 2 at NV = 1 from M = 1025 (64 workgroups of 16 waves), its 256-workgroup cap
        # from M = 16385. The last pair of a wave is ragged (first row live, second dead) for all but M - 8192 (forward), M - 1024
        # (backward at M = 1025 / 1029) waves; M = 16389 gives the forward a second trip and the backward three, the last ragged
        for M, D, stride, mode, parts in ((8197, 32, 1, 1, True), (8197, 260, 1, 0, False), (8197, 772, 1, 2, False),
                                          (77, 512, 1, 1, True), (1000, 512, 1, 2, False),
                                          (1025, 128, 4, 1, False), (1029, 128, 4, 2, True), (1025, 256, 4, 2, False), (1029, 256, 4, 1, True),
                                          (16389, 32, 1, 0, False), (16389, 32, 1, 2, True), (8192, 32, 1, 0, False), (8193, 32, 1, 1, True)):
            C("ln", M, D, groups=(1, stride, 0), mode=mode, partials=parts, tag=f"m{mode}", form=LN_FORMS[(M, D)])
        C("dec_tail", M_RG, 128, 512, groups=RG, mode=1, resid="self", partials=True)
    return tuple(out)


CASES = _cases()


def ffn_kernel_index(c):
    """launch_ffn_ln's kernel index, restated from the shape: (forward | backward | backward with lead) x (guarded | whole tiles),
    then the two head forms"""
    assert c.kind in ("ffn_fwd", "ffn_bwd")
    full = 1 if c.M % 64 == 0 else 0
    if c.proj:
        return 6 + full
    return (2 if c.lead >= 0 else (1 if c.kind == "ffn_bwd" else 0)) * 2 + full


def ln_bwd_parts(M, D):
    """mst_layernorm_bwd_parts, restated from csrc/layernorm.hip (ln_bwd_grid)"""
    nw = max(1, min(16, 32768 // (8 * D)))
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731
    wgs = cdiv(M, 4 * nw)
    if wgs < 64:
        wgs = min(cdiv(M, nw), 64)
    return min(wgs, 256)


def ln_form(backward, M, D):
    """mst_layernorm_form, restated from csrc/layernorm.hip (ln_plan) -> (NV, R, grid.x, waves per workgroup, LDS bytes). Used to lay
    out the partial rows and the kernel-order emulation without the library; where the library is at hand (the GPU test, the CPU
    completeness test) its query is asked and this restatement is only held against it"""
    cdiv = lambda a, b: (a + b - 1) // b  # noqa: E731
    nv = 1 if D <= 256 else (2 if D <= 512 else 4)
    if backward:
        nw = max(1, min(16, 32768 // (8 * D)))
        grid = ln_bwd_parts(M, D)
        return nv, (2 if nv == 1 and cdiv(M, grid * nw) > 1 else 1), grid, nw, 8 * nw * D
    grid = min(cdiv(M, 4), 2048)
    return nv, (2 if M > 4 * grid else 1), grid, 4, 0


def n_parts(c):
    return ln_bwd_parts(c.M, c.D) if c.kind == "ln" else (c.M + 63) // 64


def rows(c, spec=None):
    """-> (physical row of every logical row, number of physical rows). spec: a buffer with a row stride of its own (Buf.stride:
    logical row m at row m * stride of that buffer, whatever the case's groups say)"""
    m = np.arange(c.M, dtype=np.int64)
    if spec is not None and spec.stride:
        return m * spec.stride, c.M * spec.stride
    if c.groups is None:
        return m, c.M
    rpg, stride, off = c.groups
    return (m // rpg) * stride + off + m % rpg, ((c.M + rpg - 1) // rpg) * stride


# ------------------------------------------------------------------------------------------ buffers and stages
@dataclass(frozen=True)
class Buf:
    rows: str      # log | phys (2-D activations) | stat (1-D fp32 at the physical row) | vec (1-D fp32) | w (weights) | parts | raw
    width: int
    out: bool
    n: int = 0     # w: rows; parts: rows
    free: bool = False  # an output no stage here checks (the loss arithmetic's)
    stride: int = 0     # phys / stat: a row stride of this buffer's own (0: the case's physical rows)


@dataclass(frozen=True)
class Gemm:
    out: str
    A: str
    B: str
    K: int
    bias: str = None
    alpha: float = 1.0
    relu: bool = False
    p: float = 0.0
    site: int = 0
    self_resid: bool = False
    resid: str = None
    gate: str = None


@dataclass(frozen=True)
class LnFwd:
    h: str
    gamma: str
    beta: str
    y: str
    mean: str
    rstd: str


@dataclass(frozen=True)
class LnBwd:
    dy: object     # a buffer name, or a Gemm whose result is not stored
    x: str
    mean: str
    rstd: str
    gamma: str
    dx: str
    dxm: str
    mode: int
    p: float
    site: int
    dgamma: str
    dbeta: str
    parts: str = None


PLANS = {}  # kind -> plan function of the case kinds other modules add (tests/tail_refs.py)


def plan(c):
    """-> (buffers: name -> Buf, stages in launch order)"""
    if c.kind in PLANS:
        return PLANS[c.kind](c)
    D, F = c.D, c.F
    b, st = {}, []

    def act(name, width, out, rows_="phys"):
        b[name] = Buf(rows_, width, out)

    def stat(name, out):
        b[name] = Buf("stat", 0, out)

    def vec(name, width, out=False):
        b[name] = Buf("vec", width, out)

    def w(name, n, k):
        b[name] = Buf("w", k, False, n)

    def grads(prefix, use_parts):
        vec(prefix + "dgamma", D, True)
        vec(prefix + "dbeta", D, True)
        if use_parts:
            b[prefix + "parts"] = Buf("parts", 2 * D, True, n_parts(c))
        return prefix + "dgamma", prefix + "dbeta", (prefix + "parts" if use_parts else None)

    sr = c.resid == "self"
    if c.kind in ("ffn_fwd", "dec_tail"):
        head = c.proj or c.kind == "dec_tail"
        if head:
            act("att", D, False), act("xin", D, False), w("Wp", D, D), vec("bp", D), vec("g1", D), vec("be1", D)
            act("h1", D, True), act("x", D, True), stat("mean1", True), stat("rstd1", True)
            st += [Gemm("h1", "att", "Wp", D, bias="bp", p=c.p, site=SITE_PROJ, resid="xin"), LnFwd("h1", "g1", "be1", "x", "mean1", "rstd1")]
        else:
            act("x", D, False)
        w("W1", F, D), vec("b1", F), w("W2", D, F), vec("b2", D), vec("gamma", D), vec("beta", D)
        act("a", F, True), act("h2", D, True), act("y", D, True), stat("mean", True), stat("rstd", True)
        if c.resid == "other":
            act("r2", D, False)
        st += [Gemm("a", "x", "W1", D, bias="b1", relu=True, p=c.p, site=SITE_FF1),
               Gemm("h2", "a", "W2", F, bias="b2", p=c.p, site=SITE_FF2, self_resid=sr, resid={"x": "x", "other": "r2"}.get(c.resid)),
               LnFwd("h2", "gamma", "beta", "y", "mean", "rstd")]
        if c.kind == "dec_tail":
            # the loss launch's own arithmetic (dlogits, loss) is out of scope: dlogits is taken as the device stored it
            b["dlogits"] = Buf("log", 128, True, free=True)
            w("Wot", D, 128), w("W2t", F, D), w("W1t", D, F)
            act("dh", D, True), act("dpre", F, True), act("dh1", D, True), act("dh1m", D, True)
            g3 = grads("l3_", True)
            g1 = grads("", True)
            inv = 1.0 / (1.0 - c.p)
            st += [LnBwd(Gemm(None, "dlogits", "Wot", 128), "h2", "mean", "rstd", "gamma", "dh", None, 2, c.p, SITE_FF2, *g3),
                   Gemm("dpre", "dh", "W2t", D, alpha=inv, gate="a"),
                   LnBwd(Gemm(None, "dpre", "W1t", F), "h1", "mean1", "rstd1", "g1", "dh1", "dh1m", 1, c.p, SITE_PROJ, *g1)]
    elif c.kind == "ffn_bwd":
        w("W2t", F, D), w("W1t", D, F), act("gate", F, False), act("x", D, False), stat("mean", False), stat("rstd", False), vec("gamma", D)
        if c.lead >= 0:
            act("dyl", D, False), act("xl", D, False), stat("meanl", False), stat("rstdl", False), vec("gl", D)
            act("dh", D, True)
            if c.lead == 1:
                act("dhm", D, True)
            gl = grads("l_", c.partials)
            st.append(LnBwd("dyl", "xl", "meanl", "rstdl", "gl", "dh", "dhm" if c.lead == 1 else None, c.lead, c.p, SITE_LEAD, *gl))
            dff, resid = ("dhm" if c.lead == 1 else "dh"), ("dh" if c.resid == "x" else None)
        else:
            act("dff", D, False)
            dff, resid = "dff", None
            if c.resid == "other":
                act("r", D, False)
                resid = "r"
        act("dpre", F, True), act("dx", D, True)
        if c.mode == 1:
            act("dxm", D, True)
        g = grads("", c.partials)
        st += [Gemm("dpre", dff, "W2t", D, alpha=c.alpha, gate="gate"),
               LnBwd(Gemm(None, "dpre", "W1t", F, resid=resid), "x", "mean", "rstd", "gamma", "dx", "dxm" if c.mode == 1 else None, c.mode, c.p,
                     SITE_LN, *g)]
    elif c.kind == "gemm_ln_fwd":
        act("A", F, False, "log"), w("W", D, F), vec("gamma", D), vec("beta", D)
        if c.bias:
            vec("bias", D)
        if c.resid == "other":
            act("r", D, False, "log")
        act("h", D, True), act("y", D, True), stat("mean", True), stat("rstd", True)
        st += [Gemm("h", "A", "W", F, bias="bias" if c.bias else None, alpha=c.alpha, p=c.p, site=SITE_FF1, self_resid=sr,
                    resid="r" if c.resid == "other" else None), LnFwd("h", "gamma", "beta", "y", "mean", "rstd")]
    elif c.kind == "gemm_ln_bwd":
        act("A", F, False, "log"), w("W", D, F), vec("gamma", D), vec("bias", D), act("x", D, False), stat("mean", False), stat("rstd", False)
        if c.resid == "other":
            act("r", D, False, "log")
        act("dx", D, True)
        if c.mode == 1:
            act("dxm", D, True, "log")
        g = grads("", c.partials)
        st.append(LnBwd(Gemm(None, "A", "W", F, bias="bias", alpha=c.alpha, resid="r" if c.resid == "other" else None), "x", "mean", "rstd",
                        "gamma", "dx", "dxm" if c.mode == 1 else None, c.mode, c.p, SITE_LN, *g))
    elif c.kind == "ln":
        act("x", D, False, "log"), act("dy", D, False, "log"), vec("gamma", D), vec("beta", D)
        act("y", D, True, "log"), stat("mean", True), stat("rstd", True), act("dx", D, True, "log")
        if c.mode == 1:
            act("dxm", D, True, "log")
        g = grads("", c.partials)
        st += [LnFwd("x", "gamma", "beta", "y", "mean", "rstd"),
               LnBwd("dy", "x", "mean", "rstd", "gamma", "dx", "dxm" if c.mode == 1 else None, c.mode, c.p, SITE_LN, *g)]
    else:
        raise ValueError(c.kind)
    return b, st


# ------------------------------------------------------------------------------------------ operands
def _r16(x, dtype):
    """round an array to the activation type -> fp64"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dtype).double().numpy()


def hard_rows(g, n, width, dtype, shift=0):
    """activation rows made to be hard (fp64, 16-bit-exact): unit-scale rows; every 8th row (3, 11, ...) a common offset 8 with a
    spread of sixteenths (exact in bf16 and fp16); row 5 + shift constant (variance 0: only eps under the root); row 6 + shift small
    with one large element. (shift: the two LayerNorms of one launch get their constant rows at different rows — rstd = 316 twice
    in a chain leaves fp16's range). With fewer than 7 + shift rows: the hard rows that fit"""
    x = torch.randn((n, width), generator=g).double().numpy()
    off = np.arange(n) % 8 == 3
    k = torch.randint(-2, 3, (n, width), generator=g).double().numpy()
    x[off] = 8.0 + k[off] / 16.0
    if n > 5 + shift:
        x[5 + shift] = 3.0
    if n > 6 + shift:
        x[6 + shift] = 0.1 * x[6 + shift]
        x[6 + shift, width // 3] = 32.0
    return _r16(x, dtype)


OFFSET_ROW, CONST_ROW, SPIKE_ROW, ZERO_GAMMA, LEAD_SHIFT = 3, 5, 6, 7, 8


def _gamma(g, D):
    e = torch.rand((D,), generator=g).double().numpy() * 4.0 - 2.0      # magnitudes 0.25 .. 4
    s = np.where(torch.rand((D,), generator=g).numpy() < 0.5, -1.0, 1.0)
    v = (s * 2.0 ** e).astype(np.float32)
    v[ZERO_GAMMA] = 0.0
    return v


def _alloc(c, spec, fill):
    _, P = rows(c, spec)
    guard = GUARD if spec.out else 0
    if spec.rows in ("log", "phys"):
        return torch.full(((c.M if spec.rows == "log" else P) + guard, spec.width + PAD), fill, dtype=c.dtype)
    if spec.rows == "stat":
        return torch.full((P + guard,), fill, dtype=torch.float32)
    if spec.rows == "vec":
        return torch.full((spec.width + guard,), fill, dtype=torch.float32)
    if spec.rows == "parts":
        return torch.full((spec.n + 1, spec.width), NAN, dtype=torch.float32)
    return torch.full((spec.n, spec.width + PAD), fill, dtype=c.dtype)  # w


def owned(c, spec):
    """boolean mask over a buffer: the elements the launch owns (reads of an input, stores of an output)"""
    pm, _ = rows(c, spec)
    t = _alloc(c, spec, 0.0)
    m = np.zeros(tuple(t.shape), dtype=bool)
    if spec.rows == "log":
        m[:c.M, :spec.width] = True
    elif spec.rows == "phys":
        m[pm, :spec.width] = True
    elif spec.rows == "stat":
        m[pm] = True
    elif spec.rows == "vec":
        m[:spec.width] = True
    elif spec.rows == "parts":
        m[:spec.n] = True
    else:
        m[:, :spec.width] = True
    return m


WEIGHT_SCALE = dict(Wp=0.06, W1=0.06, W2=0.03, W2t=0.05, W1t=0.05, W=0.05, Wot=0.2)


def operands(c):
    """the case's inputs as CPU tensors, seeded, 16-bit-rounded; pad columns and the rows the launch does not own hold NaN"""
    bufs, _ = plan(c)
    pm, _ = rows(c)
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))  # (of the id: a case keeps its operands when the table grows)
    o = {}
    for name, s in bufs.items():
        if s.out:
            continue
        t = _alloc(c, s, NAN)
        if s.rows in ("log", "phys"):
            if name == "gate":     # the forward's hidden activation: ReLU and dropout leave about 60 % exact zeros
                v = torch.randn((c.M, s.width), generator=g).double().numpy()
                v = _r16(np.where(v > 0.25, v, 0.0), c.dtype)
            elif name in ("dyl", "dy", "dff"):
                v = _r16(torch.randn((c.M, s.width), generator=g).double().numpy() * 0.5, c.dtype)
            else:
                v = hard_rows(g, c.M, s.width, c.dtype, shift=LEAD_SHIFT if name == "xl" else 0)
                if name == "A":
                    v *= 0.5
            idx = np.arange(c.M) if s.rows == "log" else pm
            t[torch.from_numpy(idx), :s.width] = torch.from_numpy(v).to(c.dtype)
        elif s.rows == "w":
            t[:, :s.width] = (torch.randn((s.n, s.width), generator=g) * WEIGHT_SCALE[name]).to(c.dtype)
        elif s.rows == "vec":
            if name in ("gamma", "g1", "gl"):
                t[:] = torch.from_numpy(_gamma(g, s.width))
            else:
                t[:] = torch.randn((s.width,), generator=g) * (0.5 if name in ("beta", "be1") else 0.1)
        elif s.rows == "stat":
            continue  # below: they belong to an x
        o[name] = t
    for mean, rstd, x in (("mean", "rstd", "x"), ("meanl", "rstdl", "xl")):
        if mean in bufs and not bufs[mean].out:
            xs = gather(c, bufs[x], o[x])
            mu = xs.mean(1)
            var = ((xs - mu[:, None]) ** 2).mean(1)
            for name, v in ((mean, mu), (rstd, 1.0 / np.sqrt(var + EPS))):
                t = _alloc(c, bufs[name], NAN)
                t[torch.from_numpy(pm)] = torch.from_numpy(v).float()
                o[name] = t
    if c.kind == "dec_tail":
        o["labels"] = (torch.rand((c.M, 128), generator=g) < 0.05).to(torch.uint8)
    o["seed_word"] = torch.tensor([SEED_WORD - (1 << 64)], dtype=torch.int64)
    return o


def outputs(c):
    """the case's output buffers before the launch: SENTINEL everywhere (the parameter gradients start at INIT, partials hold NaN)"""
    bufs, _ = plan(c)
    o = {}
    for name, s in bufs.items():
        if s.out:
            o[name] = _alloc(c, s, SENTINEL)
            if s.rows == "vec":
                o[name][:s.width] = INIT
    return o


def gather(c, spec, t):
    """a buffer's logical rows as fp64 [M, width] ([M] for statistics)"""
    pm, _ = rows(c, spec)
    a = t.double().numpy()
    if spec.rows == "log":
        return a[:c.M, :spec.width]
    if spec.rows == "phys":
        return a[pm, :spec.width]
    if spec.rows == "stat":
        return a[pm]
    if spec.rows == "vec":
        return a[:spec.width]
    return a[:, :spec.width]


def scatter(c, spec, t, v):
    pm, _ = rows(c, spec)
    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(t.dtype)
    if spec.rows == "log":
        t[:c.M, :spec.width] = v
    elif spec.rows == "phys":
        t[torch.from_numpy(pm), :spec.width] = v
    elif spec.rows == "stat":
        t[torch.from_numpy(pm)] = v
    elif spec.rows == "vec":
        t[:spec.width] = v
    else:
        raise ValueError(spec.rows)


def keep_scale(c, N, p, site, counter_rows=None):
    """keep / (1 - p) of every element [M, N], decided at counter (physical row) * N + column; all ones at p = 0"""
    if p <= 0:
        return np.ones((c.M, N))
    pm = rows(c)[0] if counter_rows is None else counter_rows
    idx = pm.astype(np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    keep, scale = keep_mask(SEED ^ SEED_WORD, site, idx, p)
    return keep * scale


# ------------------------------------------------------------------------------------------ the fp64 stages and their bounds
def gemm_ref(A, B, bias, alpha, relu, k, self_resid, resid, gate):
    """-> (ref, S): the epilogue in the header's order, and the same on absolute values. k: keep / (1 - p) or None (no dropout)"""
    alpha = float(np.float32(alpha))
    t, s = A @ B.T, np.abs(A) @ np.abs(B).T
    if bias is not None:
        t, s = t + bias, s + np.abs(bias)
    t, s = t * alpha, s * abs(alpha)
    if relu:
        t = np.maximum(t, 0.0)
    if k is not None or self_resid:
        kk = 1.0 if k is None else k
        t, s = (t + t * kk, s + s * kk) if self_resid else (t * kk, s * kk)
    if resid is not None:
        t, s = t + resid, s + np.abs(resid)
    if gate is not None:
        t, s = np.where(gate > 0, t, 0.0), np.where(gate > 0, s, 0.0)
    return t, s


def gemm_bound(dtype, K, ref, S):
    uo = u_out(dtype)
    return uo * np.abs(ref) + 2.0 * (K + 16) * U * S * (1.0 + uo) + floor_(dtype)


def ln_fwd_ref(h, gamma, beta, dtype, eps=EPS):
    """-> dict of (ref, bound) for mean, rstd, y (derivation: the module's docstring)"""
    n = h.shape[1]
    uo = u_out(dtype)
    mean = h.mean(1)
    d = h - mean[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = d * rstd[:, None]
    y = xh * gamma + beta
    b_mean = (n + 16) * U * np.abs(h).mean(1)
    rel_v = (b_mean ** 2 + (n + 20) * U * (var + b_mean ** 2) + U * (var + eps)) / (var + eps)
    b_rstd = rstd * (0.5 * rel_v + 4 * U)
    e_xh = (rstd * b_mean)[:, None] + np.abs(xh) * (0.5 * rel_v + 6 * U)[:, None]
    e_y = np.abs(gamma) * e_xh + 2 * U * (np.abs(xh * gamma) + np.abs(beta))
    return dict(mean=(mean, b_mean), rstd=(rstd, b_rstd), y=(y, uo * np.abs(y) + e_y * (1 + uo) + floor_(dtype)))


def ln_bwd_ref(dy, x, mean, rstd, gamma, k, mode, dtype, e=None, init=INIT):
    """-> dict of (ref, bound) for dx, dxm (mode 1), dgamma, dbeta. k: keep / (1 - p) (ones at p = 0); e: the error dy carries
    (None: dy is a stored, 16-bit-exact tensor)"""
    M, n = dy.shape
    uo, fl = u_out(dtype), floor_(dtype)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    s1, s2 = g.mean(1), (g * xh).mean(1)
    dx = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
    ag, axh = np.abs(g), np.abs(xh)
    E = rstd[:, None] * (n + 32) * U * (ag + ag.mean(1)[:, None] + axh * (ag * axh).mean(1)[:, None])
    if e is not None:
        ge = np.abs(gamma) * e
        E = E + rstd[:, None] * (ge + ge.mean(1)[:, None] + axh * (ge * axh).mean(1)[:, None])
    out = {}
    if mode == 2:
        ref = dx * (1.0 + k)
        out["dx"] = (ref, uo * np.abs(ref) + (1.0 + k) * E * (1 + 2 * U) * (1 + uo) + fl)
    else:
        out["dx"] = (dx, uo * np.abs(dx) + E * (1 + uo) + fl)
        if mode == 1:
            ref = dx * k
            out["dxm"] = (ref, uo * np.abs(ref) + k * E * (1 + 2 * U) * (1 + uo) + fl)
    Sg, Sb = (np.abs(dy) * axh).sum(0), np.abs(dy).sum(0)
    bg = 2 * (M + 16) * U * (Sg + abs(init)) + 4 * U * Sg
    bb = 2 * (M + 16) * U * (Sb + abs(init))
    if e is not None:
        bg, bb = bg + (e * axh).sum(0), bb + e.sum(0)
    out["dgamma"] = (init + (dy * xh).sum(0), bg)
    out["dbeta"] = (init + dy.sum(0), bb)
    return out


@dataclass
class Result:
    name: str      # the stored tensor
    stage: str
    got: np.ndarray
    ref: np.ndarray
    bound: np.ndarray

    @property
    def bad(self):
        return ~(np.abs(self.got - self.ref) <= self.bound)

    @property
    def ratio(self):
        with np.errstate(invalid="ignore"):
            r = np.abs(self.got - self.ref) / np.maximum(self.bound, 1e-300)
        return float(np.max(np.where(np.isnan(r), np.inf, r)))


def _gemm_inputs(c, bufs, val, s):
    A, B = val(s.A), val(s.B)
    bias = val(s.bias) if s.bias else None
    k = keep_scale(c, B.shape[0], s.p, s.site) if s.p > 0 else None
    return A, B, bias, k, (val(s.resid) if s.resid else None), (val(s.gate) if s.gate else None)


def check(c, ins, got):
    """the stage checks in launch order -> [Result]. ins: operands(c); got: the output buffers after the launch (CPU tensors; the
    parameter gradients after their partial rows were added)"""
    bufs, stages_ = plan(c)

    def val(name):
        return gather(c, bufs[name], got[name] if bufs[name].out else ins[name])

    res = []
    for s in stages_:
        if isinstance(s, Gemm):
            A, B, bias, k, resid, gate = _gemm_inputs(c, bufs, val, s)
            ref, S = gemm_ref(A, B, bias, s.alpha, s.relu, k, s.self_resid, resid, gate)
            res.append(Result(s.out, f"gemm {s.A} x {s.B}", val(s.out), ref, gemm_bound(c.dtype, s.K, ref, S)))
        elif isinstance(s, LnFwd):
            r = ln_fwd_ref(val(s.h), val(s.gamma), val(s.beta), c.dtype)
            for key, name in (("mean", s.mean), ("rstd", s.rstd), ("y", s.y)):
                res.append(Result(name, f"ln_fwd of {s.h}", val(name), *r[key]))
        else:
            e = None
            if isinstance(s.dy, Gemm):
                q = s.dy
                A, B, bias, k, resid, gate = _gemm_inputs(c, bufs, val, q)
                dy, S = gemm_ref(A, B, bias, q.alpha, q.relu, k, q.self_resid, resid, gate)
                e = gemm_bound(c.dtype, q.K, dy, S)
                label = f"ln_bwd of gemm {q.A} x {q.B}"
            else:
                dy, label = val(s.dy), f"ln_bwd of {s.dy}"
            r = ln_bwd_ref(dy, val(s.x), val(s.mean), val(s.rstd), val(s.gamma), keep_scale(c, c.D, s.p if s.mode else 0.0, s.site), s.mode,
                           c.dtype, e)
            for key, name in (("dx", s.dx), ("dxm", s.dxm), ("dgamma", s.dgamma), ("dbeta", s.dbeta)):
                if name is not None:
                    res.append(Result(name, label, val(name), *r[key]))
    return res


def describe(c, r):
    """a failed Result in words: the tensor, how many elements, the worst one, where they lie"""
    bad = np.atleast_2d(r.bad.T).T if r.bad.ndim == 1 else r.bad
    got, ref, bound = (np.atleast_2d(x.T).T if x.ndim == 1 else x for x in (r.got, r.ref, r.bound))
    with np.errstate(invalid="ignore"):
        ratio = np.where(bad, np.abs(got - ref) / np.maximum(bound, 1e-300), 0)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    rr, cc = np.nonzero(bad)
    return (f"{c.id}: {r.name} ({r.stage}): {int(bad.sum())}/{bad.size} elements outside the bound; worst at row {i}, column {j}: got "
            f"{got[i, j]!r}, want {ref[i, j]!r}, bound {bound[i, j]:.3g} ({ratio[i, j]:.3g} bounds); rows {rr.min()}..{rr.max()}, columns "
            f"{cc.min()}..{cc.max()}, {len(np.unique(rr))} rows, {len(np.unique(cc))} columns, tiles (row // 64) {sorted(set((rr // 64).tolist()))[:12]}")


def intact(c, got):
    """what the launch must leave alone and must have filled -> list of complaints (empty: all well)"""
    bufs, _ = plan(c)
    out = []
    for name, s in bufs.items():
        if not s.out:
            continue
        a = got[name].double().numpy()
        own = owned(c, s)
        if s.rows == "parts":
            if np.isnan(a[own]).any():
                out.append(f"{name}: NaN left in {int(np.isnan(a[own]).any(1).sum())} of the {s.n} partial rows the launch owns")
            if not np.isnan(a[~own]).all():
                out.append(f"{name}: the guard row of partials was written")
            continue
        if not np.isfinite(a[own]).all():
            rr = np.nonzero(~np.isfinite(a) & own)[0]
            out.append(f"{name}: {len(rr)} non-finite owned elements (a NaN pad column or a row outside the groups was read), rows {rr.min()}..{rr.max()}")
        if not (a[~own] == SENTINEL).all():
            idx = np.argwhere((a != SENTINEL) & ~own)
            out.append(f"{name}: {len(idx)} elements outside the output were written (pad columns, guard rows, rows outside the groups); "
                       f"first at {tuple(idx[0])}, buffer shape {a.shape}")
    return out
