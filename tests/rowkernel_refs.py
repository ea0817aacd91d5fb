"""Plain fp64 references (no GPU, no library) of the stand-alone row kernels of csrc/embed.hip and of mst_segment_sumsq, the bounds they
are held to, and the tables of cases: mst_embed_fwd, mst_embed_bwd, mst_group_colsum, mst_mask_from_lengths, mst_segment_sumsq.

BUFFERS. Every 2-D buffer is PAD columns wider than the kernel is told (the leading dimension) where the case says so, every output has
GUARD rows behind it; what the launch does not own holds NaN in an input and SENTINEL in an output (fp32 gradients, which are
ACCUMULATED INTO, start at random values inside and SENTINEL outside). intact() complains about a NaN that was read and a sentinel that
was overwritten.

BOUNDS, derived per element (u = 2^-24; gamma_n = n u / (1 - n u), the classical bound of n roundings in ANY order):
  embed_fwd   out = alpha (e + c) + p in fp32, then one 16-bit store. fl(e + c) is one rounding; alpha * s + p is one rounding where the
              compiler contracts it to an fma and two where it does not: at most three, each relative to a partial result no larger
              than S = |alpha| (|e| + |c|) + |p|. E = 4 u S covers both forms with one to spare. The store adds half an ulp of the 16-bit
              type, taken at |ref| + E (the fp32 value may lie in the next binade): bound = half_ulp(|ref| + E) + E.
  keymask, mask_from_lengths   exact.
  embed_bwd dtable[v, d]  = init + sum over the n kept positions r with tok[r] = v of fl(alpha dX[r, d]), added by fp32 atomics in
              no fixed order: n additions and one product rounding per term: gamma_(n + 1) (|init| + sum |alpha dX|). n = 0: exact (the
              element is never touched).
  dcls / group_colsum dst[k, d] = init + alpha sum over the samples b of class k and t < T of X[b, s_off + t, d]: per-thread sums of
              every RG-th row, RG partial sums through LDS, one product with alpha, one atomic per workgroup: n = (samples) T addends
              in some order, one product, one more addition: gamma_(n + 2) (|init| + |alpha| sum |X|).
  segment_sumsq out[i] = sum x^2 over hi - lo terms: one rounding per square (none where it is contracted), n additions in the order
              of 256 threads, a butterfly and four waves: gamma_(n + 1) sum x^2, plus n 2^-126 for squares below fp32's normal range
              (whether or not the device flushes them). A segment holding an inf: inf. An empty segment: 0.
None of these sums is promised to repeat bit for bit (atomics), and none is asserted to.
No constant was chosen after looking at a GPU result."""
import os
import sys
import zlib
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_refs import BF, FP, DTYPES, DT_NAME, SENTINEL  # noqa: E402,F401
from rowblock_refs import Result  # noqa: E402,F401

U = 2.0 ** -24
PAD, GUARD = 8, 2
NAN = float("nan")
MASK_SENTINEL = 7          # uint8 masks before a launch
V, NCLS = 11, 3            # vocabulary and class-table rows of the embedding cases; class 1 is never used
NAN_TOKEN = V - 2          # the table row that holds NaN where a case says so: referenced by dropped positions only
MANT = {BF: 8, FP: 11}
EMIN = {BF: -126, FP: -14}


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def half_ulp(v, dtype):
    """half the spacing of `dtype` at |v| (below the smallest normal: half the subnormal spacing)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** EMIN[dtype])))
    return 2.0 ** (e - MANT[dtype])


def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _r16(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dtype)


# ------------------------------------------------------------------------------------------ embedding
@dataclass(frozen=True)
class Embed:
    dtype: torch.dtype
    B: int
    T: int
    D: int
    s_off: int = 0
    extra: int = 0          # rows of every sample behind s_off + T (S_out = s_off + T + extra)
    pad: bool = True        # ldt = D + 4, ldc = D + 8, ldp = D + 12, ld_out = D + 8 instead of D
    cls: bool = True        # forward: cls_table given; backward: dcls given where D allows it (D % 8 == 0)
    keymask: bool = True
    keep: str = None        # None | "some" (three in ten dropped) | "sample" (also every position of sample 1)
    tokens: str = "mixed"   # mixed (0, V - 1, a run of one id over the last sample) | runs (runs of 300) | equal (one id everywhere)
    nan_row: bool = False   # table row NAN_TOKEN holds NaN; needs keep
    fwd: bool = True        # False: a case of the backward only
    tag: str = ""

    @property
    def id(self):
        return f"embed-{DT_NAME[self.dtype]}-B{self.B}-T{self.T}-D{self.D}-s{self.s_off}" + (f"-{self.tag}" if self.tag else "")

    @property
    def S_out(self):
        return self.s_off + self.T + self.extra

    @property
    def alpha(self):
        return float(np.float32(np.sqrt(self.D)))

    @property
    def dcls(self):
        return self.cls and self.D % 8 == 0

    def ld(self, which):
        return self.D + ({"t": 4, "c": 8, "p": 12, "o": 8}[which] if self.pad else 0)


def _embed_cases():
    out = []
    for dt in DTYPES:
        E = lambda *a, **k: out.append(Embed(dt, *a, **k))  # noqa: E731
        E(3, 7, 4, s_off=0, extra=0, pad=False, cls=False, tag="plain")                       # nothing optional, dense
        E(4, 9, 40, s_off=1, extra=2, keep="sample", nan_row=True, tag="keep-cls")             # everything optional at once
        E(2, 5, 256, s_off=0, extra=2, keymask=False, tag="nomask")                           # one full trip of the d loop
        E(2, 5, 260, s_off=1, extra=1, keep="some", nan_row=True, tag="keep")                  # d += 256: a second trip of one lane
        E(2, 3, 1024, s_off=1, extra=0, tag="wide")                                            # four whole trips
        E(7, 2341, 8, s_off=0, extra=1, keep="some", tokens="runs", tag="gridstride")          # B T = 16387 > 4 * 4096 rows
        E(2, 6, 12, s_off=1, extra=1, cls=False, fwd=False, tag="bwd-nodcls")                  # backward without dcls at D % 8 != 0
        E(8, 64, 40, s_off=0, extra=0, tokens="equal", fwd=False, tag="bwd-collide")           # 512 atomics on every element of one row
    return tuple(out)


EMBED_CASES = _embed_cases()


def embed_operands(c):
    g = _gen(c.id)
    B, T, D, S = c.B, c.T, c.D, c.S_out
    if c.tokens == "equal":
        tok = np.full((B, T), 4, dtype=np.int32)
    elif c.tokens == "runs":
        tok = ((np.arange(B * T) // 300) % V).astype(np.int32).reshape(B, T)
        tok[0, :50] = torch.randint(0, V, (50,), generator=g).numpy()
    else:
        tok = torch.randint(0, V, (B, T), generator=g).numpy().astype(np.int32)
        tok[-1, :] = 5
        tok[0, 0], tok[0, 1], tok[0, 2] = 0, V - 1, NAN_TOKEN
    keep = None
    if c.keep:
        keep = (torch.rand((B, T), generator=g).numpy() < 0.7).astype(np.uint8)
        if c.keep == "sample":
            keep[1, :] = 0
        keep[0, 0], keep[0, 1] = 1, 0
    if c.nan_row:
        assert keep is not None
        keep[tok == NAN_TOKEN] = 0

    def f32(rows, width, ld, scale=1.0):
        t = torch.full((rows, ld), NAN, dtype=torch.float32)
        t[:, :width] = torch.randn((rows, width), generator=g) * scale
        return t

    o = dict(tokens=torch.from_numpy(tok), table=f32(V, D, c.ld("t")), pos=f32(S, D, c.ld("p")),
             classes=torch.from_numpy(np.array([0, 2] * B, dtype=np.int32)[:B].copy()))
    if c.nan_row:
        o["table"][NAN_TOKEN] = NAN
    own = np.zeros(S, dtype=bool)
    own[c.s_off:c.s_off + T] = True
    o["pos"][torch.from_numpy(~own)] = NAN
    if c.cls:
        o["cls_table"] = f32(NCLS, D, c.ld("c"), 0.5)
    if keep is not None:
        o["keep"] = torch.from_numpy(keep.reshape(-1).copy())
    dX = torch.full((B * S + GUARD, c.ld("o")), NAN, dtype=c.dtype)
    rows_ = (np.arange(B)[:, None] * S + c.s_off + np.arange(T)[None, :]).reshape(-1)
    dX[torch.from_numpy(rows_), :D] = (torch.randn((B * T, D), generator=g) * 0.5).to(c.dtype)
    o["dX"] = dX
    return o


def embed_rows(c):
    """flat row of out / dX / keymask of every (b, t) -> [B * T]"""
    return (np.arange(c.B)[:, None] * c.S_out + c.s_off + np.arange(c.T)[None, :]).reshape(-1)


def embed_fwd_outputs(c):
    o = dict(out=torch.full((c.B * c.S_out + GUARD, c.ld("o")), SENTINEL, dtype=c.dtype))
    if c.keymask:
        o["keymask"] = torch.full((c.B * c.S_out + GUARD,), MASK_SENTINEL, dtype=torch.uint8)
    return o


def embed_bwd_outputs(c):
    g = _gen(c.id + "/grads")
    o = {}
    for name, rows_, ld in (("dtable", V, c.ld("t")), ("dcls", NCLS, c.ld("c"))):
        if name == "dcls" and not c.dcls:
            continue
        t = torch.full((rows_ + GUARD, ld), SENTINEL, dtype=torch.float32)
        t[:rows_, :c.D] = torch.randn((rows_, c.D), generator=g)
        o[name] = t
    return o


def _kept(c, ins):
    return np.ones(c.B * c.T, dtype=bool) if "keep" not in ins else ins["keep"].numpy().astype(bool)


def embed_fwd_check(c, ins, got):
    """-> [Result] of out (its B T owned rows) and keymask"""
    D = c.D
    tok = ins["tokens"].numpy().reshape(-1)
    b = np.arange(c.B * c.T) // c.T
    t = np.arange(c.B * c.T) % c.T
    kept = _kept(c, ins)
    table = ins["table"].double().numpy()[:, :D]
    e = np.where(kept[:, None], table[np.where(kept, tok, 0)], 0.0)   # a dropped position takes a zero row: its table row is not read
    cc = ins["cls_table"].double().numpy()[ins["classes"].numpy()[b], :D] if c.cls else np.zeros_like(e)
    p = ins["pos"].double().numpy()[c.s_off + t, :D]
    a = c.alpha
    ref = a * (e + cc) + p
    E = 4 * U * (abs(a) * (np.abs(e) + np.abs(cc)) + np.abs(p))
    rows_ = embed_rows(c)
    res = [Result("out", "embed_fwd", got["out"].double().numpy()[rows_, :D], ref, half_ulp(np.abs(ref) + E, c.dtype) + E)]
    if c.keymask:
        res.append(Result("keymask", "embed_fwd", got["keymask"].double().numpy()[rows_], (tok != 0).astype(np.float64), np.zeros(len(tok))))
    return res


def colsum_ref(X, idx, n_dst, T, s_off, S_out, alpha, init):
    """X: fp64 [B * S_out (+ guard), D] -> (ref, bound) of dst[n_dst, D] += alpha sum_t X[b, s_off + t]"""
    B, D = len(idx), X.shape[1]
    Xb = X[:B * S_out].reshape(B, S_out, D)[:, s_off:s_off + T]
    a = float(np.float32(alpha))
    s, sa, n = np.zeros((n_dst, D)), np.zeros((n_dst, D)), np.zeros(n_dst)
    np.add.at(s, idx, Xb.sum(1))
    np.add.at(sa, idx, np.abs(Xb).sum(1))
    np.add.at(n, idx, T)
    return init + a * s, np.where(n[:, None] > 0, gamma(n + 2)[:, None] * (np.abs(init) + abs(a) * sa), 0.0)


def embed_bwd_check(c, ins, before, got):
    """before: the gradient buffers as embed_bwd_outputs made them -> [Result] of dtable and, where given, dcls"""
    D = c.D
    tok = ins["tokens"].numpy().reshape(-1)
    kept = _kept(c, ins)
    a = c.alpha
    dX = ins["dX"].double().numpy()[:, :D]
    rows_ = embed_rows(c)
    init = before["dtable"].double().numpy()[:V, :D]
    s, sa, n = np.zeros((V, D)), np.zeros((V, D)), np.zeros(V)
    np.add.at(s, tok[kept], a * dX[rows_[kept]])
    np.add.at(sa, tok[kept], np.abs(a * dX[rows_[kept]]))
    np.add.at(n, tok[kept], 1)
    res = [Result("dtable", "embed_bwd", got["dtable"].double().numpy()[:V, :D], init + s,
                  np.where(n[:, None] > 0, gamma(n + 1)[:, None] * (np.abs(init) + sa), 0.0))]
    if c.dcls:
        init = before["dcls"].double().numpy()[:NCLS, :D]
        ref, bound = colsum_ref(dX, ins["classes"].numpy(), NCLS, c.T, c.s_off, c.S_out, a, init)
        res.append(Result("dcls", "embed_bwd", got["dcls"].double().numpy()[:NCLS, :D], ref, bound))
    return res


def intact2d(name, t, rows_, width, sentinel=SENTINEL):
    """an output buffer [rows + guard, ld]: its owned rows x width are finite, everything else still holds the sentinel"""
    a = t.double().numpy()
    own = np.zeros(a.shape, dtype=bool)
    if a.ndim == 1:
        own[rows_] = True
    else:
        own[np.asarray(rows_)[:, None], np.arange(width)[None, :]] = True
    out = []
    if not np.isfinite(a[own]).all():
        out.append(f"{name}: {int((~np.isfinite(a) & own).sum())} non-finite owned elements (a NaN pad column, guard row or dropped table row was read)")
    if not (a[~own] == sentinel).all():
        idx = np.argwhere((a != sentinel) & ~own)
        out.append(f"{name}: {len(idx)} elements outside the output were written; first at {tuple(idx[0])}, buffer shape {a.shape}")
    return out


def embed_fwd_intact(c, got):
    out = intact2d("out", got["out"], embed_rows(c), c.D)
    if c.keymask:
        out += intact2d("keymask", got["keymask"], embed_rows(c), 0, MASK_SENTINEL)
    return out


def embed_bwd_intact(c, got):
    out = intact2d("dtable", got["dtable"], np.arange(V), c.D)
    if c.dcls:
        out += intact2d("dcls", got["dcls"], np.arange(NCLS), c.D)
    return out


# ------------------------------------------------------------------------------------------ group_colsum
@dataclass(frozen=True)
class Colsum:
    dtype: torch.dtype
    B: int
    T: int
    D: int
    s_off: int
    extra: int
    pad: bool               # ldd = D + 8, ldx = D + 8
    alpha: float
    one_class: bool         # every sample in class 2 (else classes 0 and 2); class 1 is never used either way
    form: tuple             # (cpr, RG, grid.x, LDS bytes) the case is in the table for

    @property
    def id(self):
        return f"colsum-{DT_NAME[self.dtype]}-T{self.T}-D{self.D}-s{self.s_off}" + ("-one" if self.one_class else "")

    @property
    def S_out(self):
        return self.s_off + self.T + self.extra


COLSUM_D = (8, 24, 40, 256, 1032, 2048)
COLSUM_T = (1, 63, 64, 65, 130)
# D -> (cpr, RG), written out: cpr = D / 8 chunks of 16 bytes per row, RG = floor(256 / cpr) row groups
COLSUM_MAP = {8: (1, 256), 24: (3, 85), 40: (5, 51), 256: (32, 8), 1032: (129, 1), 2048: (256, 1)}


def _colsum_cases():
    out = []
    for dt in DTYPES:
        for i, D in enumerate(COLSUM_D):
            for j, T in enumerate(COLSUM_T):
                cpr, rg = COLSUM_MAP[D]
                out.append(Colsum(dt, 3, T, D, s_off=(i + j) % 2, extra=(i + 2 * j) % 3, pad=(i + j) % 3 != 0, alpha=1.0 if (i, j) == (0, 0) else -1.75,
                                  one_class=(i + j) % 4 == 1, form=(cpr, rg, (T + 63) // 64, 4 * rg * D)))
    return tuple(out)


COLSUM_CASES = _colsum_cases()


def colsum_operands(c):
    g = _gen(c.id)
    ld = c.D + (PAD if c.pad else 0)
    X = torch.full((c.B * c.S_out + GUARD, ld), NAN, dtype=c.dtype)
    rows_ = (np.arange(c.B)[:, None] * c.S_out + c.s_off + np.arange(c.T)[None, :]).reshape(-1)
    X[torch.from_numpy(rows_), :c.D] = torch.randn((c.B * c.T, c.D), generator=g).to(c.dtype)
    idx = np.full(c.B, 2, dtype=np.int32) if c.one_class else np.array([0, 2, 0], dtype=np.int32)
    return dict(X=X, idx=torch.from_numpy(idx))


def colsum_outputs(c):
    g = _gen(c.id + "/dst")
    t = torch.full((NCLS + GUARD, c.D + (PAD if c.pad else 0)), SENTINEL, dtype=torch.float32)
    t[:NCLS, :c.D] = torch.randn((NCLS, c.D), generator=g)
    return dict(dst=t)


def colsum_check(c, ins, before, got):
    init = before["dst"].double().numpy()[:NCLS, :c.D]
    ref, bound = colsum_ref(ins["X"].double().numpy()[:, :c.D], ins["idx"].numpy(), NCLS, c.T, c.s_off, c.S_out, c.alpha, init)
    return [Result("dst", "group_colsum", got["dst"].double().numpy()[:NCLS, :c.D], ref, bound)]


# ------------------------------------------------------------------------------------------ mask_from_lengths
@dataclass(frozen=True)
class Mask:
    B: int
    S: int
    add: int

    @property
    def id(self):
        return f"mask-B{self.B}-S{self.S}-add{self.add}"

    @property
    def lens(self):
        S = self.S
        return np.array(([0, 1, S - 1, S, S + 3] * self.B)[(self.S % 5):][:self.B], dtype=np.int32)


# B S = 255, 256, 257 and 3 * 256 + 1 (257 and 769 are primes: one long row)
MASK_CASES = tuple(Mask(B, S, add) for B, S in ((5, 51), (8, 32), (1, 257), (1, 769)) for add in (-1, 0, 1))


def mask_ref(c):
    return (np.arange(c.S)[None, :] < (c.lens.astype(np.int64)[:, None] + c.add)).astype(np.uint8)


# ------------------------------------------------------------------------------------------ segment_sumsq
@dataclass(frozen=True)
class Seg:
    n: int

    @property
    def id(self):
        return f"segsumsq-n{self.n}"


SEG_CASES = (Seg(1), Seg(300))
SEG_WIDE, SEG_INF = (0, 1000), (1000, 1100)   # the element ranges that hold the 1e-20 .. 1e18 values and the inf
SEG_N = 24000


def seg_operands(c):
    """-> x fp32 [SEG_N + 1] (its last element NaN: behind every range), ranges int64 [n, 2]"""
    g = _gen("segment_sumsq")
    x = torch.randn((SEG_N + 1,), generator=g)
    mag = 10.0 ** (torch.rand((1000,), generator=g).double() * 37.0 - 20.0)   # 1e-20 .. 1e17
    sign = torch.where(torch.rand((1000,), generator=g) < 0.5, -1.0, 1.0)
    x[:1000] = (mag * sign).float()
    x[0], x[1] = 1e-20, 1e18
    x[1050] = float("inf")
    x[SEG_N] = NAN
    if c.n == 1:
        return dict(x=x, ranges=torch.tensor([[1103, 6103]], dtype=torch.int64))
    lo = 1100
    r = [SEG_WIDE, SEG_INF, (lo, lo), (lo + 1, lo + 2), (lo + 3, lo + 258), (lo + 3, lo + 259), (lo + 5, lo + 262), (lo + 7, lo + 5007),
         (lo + 100, lo + 4000), (SEG_N - 256, SEG_N), (SEG_N, SEG_N)]
    gg = _gen("segment_sumsq/ranges")
    while len(r) < c.n:
        a = int(torch.randint(lo, SEG_N - 700, (1,), generator=gg))
        r.append((a, a + int(torch.randint(0, 700, (1,), generator=gg))))
    return dict(x=x, ranges=torch.tensor(r, dtype=torch.int64))


def seg_check(ins, got):
    """-> (Result over the finite segments, got and want of the segments holding an inf)"""
    x = ins["x"].double().numpy()
    sq = x * x
    rr = ins["ranges"].numpy()
    ref = np.array([sq[a:b].sum() for a, b in rr])
    n = np.array([b - a for a, b in rr], dtype=np.float64)
    fin = np.isfinite(ref)
    bound = gamma(n + 1) * np.where(fin, ref, 0.0) + n * 2.0 ** -126
    g = got.double().numpy()[:len(rr)]
    return Result("out", "segment_sumsq", g[fin], ref[fin], bound[fin]), g[~fin], ref[~fin]


# ------------------------------------------------------------------------------------------ refusals
ARGS = {
    "mst_embed_fwd": "dtype B T D tokens table ldt classes cls_table ldc pos ldp alpha out ld_out S_out s_off keymask keep stream",
    "mst_embed_bwd": "dtype B T D tokens dtable ldt classes dcls ldc alpha dX ld_dx S_out s_off keep stream",
    "mst_group_colsum": "dtype B T D X ldx S_out s_off idx dst ldd alpha stream",
    "mst_mask_from_lengths": "B S lens add keymask stream",
    "mst_segment_sumsq": "x ranges n_segments out stream",
    "mst_group_colsum_form": "T D form",
}
INVALID, UNSUPPORTED = -1, -3
ODD = "odd"   # in place of a pointer: the good pointer plus 2 bytes (not 16-byte aligned)
# (entry point, arguments changed from a good call, status, fragment of mst_last_error()). Every MST_CHECK_ARG of the entry points of
# csrc/embed.hip and of mst_segment_sumsq once (the compound ones once per clause that matters), in the order of the source
REFUSALS = (
    ("mst_embed_fwd", dict(D=6, ldt=8, ldp=8, ld_out=8), INVALID, "D a multiple of 4"),
    ("mst_embed_fwd", dict(B=0), INVALID, "B,T,D must be positive"),
    ("mst_embed_fwd", dict(pos=None), INVALID, "mst_embed_fwd: null pointer"),
    ("mst_embed_fwd", dict(classes=None), INVALID, "cls_table needs classes"),
    ("mst_embed_fwd", dict(ldp=18), INVALID, "leading dims must be multiples of 4"),
    ("mst_embed_fwd", dict(ldc=18), INVALID, "leading dims must be multiples of 4"),
    ("mst_embed_fwd", dict(s_off=2), INVALID, "rows do not fit in S_out"),
    ("mst_embed_fwd", dict(s_off=-1), INVALID, "rows do not fit in S_out"),
    ("mst_embed_fwd", dict(dtype=2), UNSUPPORTED, "unsupported activation dtype 2"),
    ("mst_embed_bwd", dict(T=0), INVALID, "mst_embed_bwd: B,T,D must be positive"),
    ("mst_embed_bwd", dict(dX=None), INVALID, "mst_embed_bwd: null pointer"),
    ("mst_embed_bwd", dict(classes=None), INVALID, "dcls needs classes"),
    # the column sums' checks, which used to come AFTER the scatter launch had added to dtable
    ("mst_embed_bwd", dict(D=12), INVALID, "D must be a multiple of 8"),
    ("mst_embed_bwd", dict(D=2056), INVALID, "D must be a multiple of 8 (<= 2048)"),
    ("mst_embed_bwd", dict(ld_dx=20), INVALID, "rows 16-byte aligned"),
    ("mst_embed_bwd", dict(dX=ODD), INVALID, "rows 16-byte aligned"),
    ("mst_embed_bwd", dict(B=65536), INVALID, "B too large for grid.y"),
    ("mst_embed_bwd", dict(dtype=2), UNSUPPORTED, "unsupported activation dtype 2"),
    ("mst_group_colsum", dict(idx=None), INVALID, "mst_group_colsum: bad argument"),
    ("mst_group_colsum", dict(T=0), INVALID, "mst_group_colsum: bad argument"),
    ("mst_group_colsum", dict(B=65536), INVALID, "B too large for grid.y"),
    ("mst_group_colsum", dict(D=12), INVALID, "D must be a multiple of 8"),
    ("mst_group_colsum", dict(D=2056), INVALID, "(<= 2048)"),
    ("mst_group_colsum", dict(ldx=20), INVALID, "rows 16-byte aligned"),
    ("mst_group_colsum", dict(X=ODD), INVALID, "rows 16-byte aligned"),
    ("mst_group_colsum", dict(dtype=2), UNSUPPORTED, "unsupported activation dtype 2"),
    ("mst_mask_from_lengths", dict(B=0), INVALID, "mst_mask_from_lengths: bad argument"),
    ("mst_mask_from_lengths", dict(lens=None), INVALID, "mst_mask_from_lengths: bad argument"),
    ("mst_segment_sumsq", dict(n_segments=0), INVALID, "mst_segment_sumsq: bad argument"),
    ("mst_segment_sumsq", dict(n_segments=65536), INVALID, "mst_segment_sumsq: bad argument"),
    ("mst_segment_sumsq", dict(ranges=None), INVALID, "mst_segment_sumsq: bad argument"),
    ("mst_group_colsum_form", dict(form=None), INVALID, "mst_group_colsum_form: null form"),
    ("mst_group_colsum_form", dict(T=0), INVALID, "mst_group_colsum: bad argument"),
    ("mst_group_colsum_form", dict(D=12), INVALID, "D must be a multiple of 8"),
)
# the good call every refusal departs from: B = 2, T = 3, D = 16, S_out = 4, s_off = 1, every leading dimension 16; pointer arguments are
# named here and supplied by the test (device buffers on the GPU, any non-NULL 16-byte-aligned number where no launch can follow)
REFUSAL_SHAPE = dict(dtype=0, B=2, T=3, D=16, S=4, ldt=16, ldc=16, ldp=16, ld_out=16, ld_dx=16, ldx=16, ldd=16, S_out=4, s_off=1,
                     alpha=1.0, add=0, n_segments=2, stream=None)
POINTERS = ("tokens table classes cls_table pos out keymask keep dtable dcls dX X idx dst lens x ranges form").split()


def refusal_args(entry, changes, pointers):
    """the argument list of one refused call. pointers: name -> integer address of a good buffer"""
    vals = dict(REFUSAL_SHAPE)
    vals.update(pointers)
    for k, v in changes.items():
        vals[k] = (pointers[k] + 2) if v == ODD else v
    return [vals[name] for name in ARGS[entry].split()]
