"""A plain fp64 reference of mst_gemm_wgrad_batch_flush (no GPU, no library), the tolerance it is held to, and the table of batches
that reaches every launch form the flush can take (mst_gemm_wgrad_plan in include/mst_hip.h).

The operation (include/mst_hip.h, mst_wgrad_args), per problem of a batch, on the 16-bit-rounded (or uint8) operands:
    dW[n, k] += scale * sum_m A[m, n] B[m, k]        db[n] += scale * sum_m A[m, n]
with the rows of A and of B optionally remapped (logical row m at physical row (m / rpg) * stride + offset + m % rpg).

A case is one whole batch, because the form is a property of the batch (the total of N * K decides the tile, the work items decide
the M split, and the scratch buffer's size decides between fp32 atomics and the two-pass reduction). Every case records the plan it
is meant to get; tests/test_wgrad_refs_cpu.py asks the library's own decision for it."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

BF, FP = torch.bfloat16, torch.float16
DTYPES = (BF, FP)
DT_NAME = {BF: "bf16", FP: "fp16"}
MODES = ("int", "real")
SENTINEL = 7.0
TILE = {0: (64, 64), 1: (128, 128), 2: (256, 128), 3: (256, 256)}  # form -> (BN, BK)
THRESHOLDS = (128 * 128 * 24, 256 * 128 * 36, 256 * 256 * 24)     # 393,216 / 1,179,648 / 1,572,864 outputs: forms 1, 2, 3 begin
SLOTS = (1024, 512, 256, 256)                                       # work items of one resident round, per form
STAGE = 64                                                          # rows of one LDS stage
SLOT_BYTES, BIAS_ROW_BYTES = 256 * 256 * 4, 256 * 4                 # scratch per work item: its tile, its bias row


def roundup(a, b):
    return (a + b - 1) // b * b


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------ slab arithmetic, restated
def m_chunk(M, split):
    """rows of one M slab: roundup64(cdiv(M, split))"""
    return roundup(cdiv(M, split), STAGE)


def slab_rows(M, split):
    """row counts of the slabs that own rows (the others exit at once)"""
    mc = m_chunk(M, split)
    return [min(mc, M - s * mc) for s in range(split) if s * mc < M]


def whole_stages(M, split):
    """every slab of the problem is whole 64-row stages (what the interleaved main loop needs; else its last slab is ragged)"""
    return all(r % STAGE == 0 for r in slab_rows(M, split))


# ------------------------------------------------------------------------------------------ problems and batches
@dataclass(frozen=True)
class Prob:
    kind: str
    M: int
    N: int
    K: int
    ta: int = 0           # A row remap: logical rows are rows 1..ta of every ta + 1 physical rows (0: none)
    tb: int = 0           # the same for B
    db: bool = True
    scale: float = 1.0
    a_u8: bool = False
    pad: int = 0          # columns of A and B behind roundup8(N) / roundup8(K): never read, hold NaN

    @property
    def lda(self):
        return roundup(self.N, 8) + self.pad

    @property
    def ldb(self):
        return roundup(self.K, 8) + self.pad

    @property
    def ldw(self):
        return self.K + 4

    def rows(self, t):
        assert not t or self.M % t == 0
        return self.M // t * (t + 1) if t else self.M

    def phys(self, t):
        """physical row of every logical row under a remap of group size t"""
        m = np.arange(self.M, dtype=np.int64)
        return (m // t) * (t + 1) + 1 + m % t if t else m

    def remap(self, t):
        return (t, t + 1, 1) if t else (0, 0, 0)

    def body(self, narrow):
        """the kernel body the problem runs: 16-bit or uint8 A, on the narrow 256 x 128 tile inside form 3 or the form's own"""
        return ("narrow-" if narrow else "") + ("u8" if self.a_u8 else "16")

    @property
    def remap_kind(self):
        if self.ta and self.ta < STAGE:
            return "divided"
        if self.ta:
            return "carried"
        return "b-only" if self.tb else "none"


def _kinds(form):
    """the problem kinds of the table, N and K relative to the form's tile"""
    bn, bk = TILE[form]
    if form == 0:
        rag, mix_n, mix_k = (70, 36), 100, 90
    else:
        rag, mix_n, mix_k = (300, 200), bn + (72 if form == 1 else 44), bk + (52 if form < 3 else 44)
    return [
        Prob("interior", 512, 2 * bn, 2 * bk),
        Prob("ragged", 500, rag[0], rag[1], scale=0.5, pad=8),
        Prob("carried", 512, mix_n, mix_k, ta=128, tb=128),
        Prob("group64", 512, mix_n, mix_k, ta=64, db=False, scale=2.0),
        Prob("divided", 264, mix_n, mix_k, ta=33, tb=33, scale=0.5),
        Prob("b-only", 500, mix_n, mix_k, tb=100, scale=2.0),
        Prob("u8", 512, 128, bk, tb=128, db=False, scale=2.0, a_u8=True),
        Prob("u8-frames", 512, 40, bk, tb=128, scale=2.0, a_u8=True),
        Prob("stage", 64, bn, bk),
        Prob("part-stage", 40, bn, bk),
    ]


def _fill(M, N, K):
    return Prob("filler", M, N, K)


BATCHES = {
    0: tuple(_kinds(0) + [_fill(512, 128, 64)]),
    1: tuple(_kinds(1) + [_fill(512, 256, 256), _fill(520, 256, 256)]),
    2: tuple(_kinds(2) + [_fill(512, 512, 512), _fill(512, 512, 512), _fill(520, 512, 512)]),
    # the whole-step form: problems with K <= 128 run the narrow body in the same launch
    3: tuple(_kinds(3) + [Prob("narrow", 512, 512, 128), Prob("narrow-ragged", 500, 300, 72, scale=0.5, pad=8),
                          Prob("narrow-u8", 512, 128, 128, tb=128, db=False, scale=2.0, a_u8=True),
                          _fill(512, 512, 512), _fill(520, 512, 512), _fill(512, 256, 512)]),
}


@dataclass(frozen=True)
class Plan:
    form: int
    narrow: int
    items: int
    two_pass: int
    splits: tuple


# What the flush is meant to decide for each batch without a scratch buffer. Every split is min(S, cdiv(M, 128)) with S = cdiv(max M,
# 128) = 4 in form 0 and 5 (a 520-row filler) in forms 1..3, since sum(tiles * split) stays inside the form's resident round; the
# narrow problems of form 3 (bits 10..12) get (5 * 5 + 4) / 8 = 3. items = sum(tiles * split).
_PLANS = {
    0: Plan(0, 0, 106, 0, (4, 4, 4, 4, 3, 4, 4, 4, 1, 1, 4)),
    1: Plan(1, 0, 146, 0, (4, 4, 4, 4, 3, 4, 4, 4, 1, 1, 4, 5)),
    2: Plan(2, 0, 206, 0, (4, 4, 4, 4, 3, 4, 4, 4, 1, 1, 4, 4, 5)),
    3: Plan(3, 0b111 << 10, 153, 0, (4, 4, 4, 4, 3, 4, 4, 4, 1, 1, 3, 3, 3, 4, 5, 4)),
}
SCRATCH_MODES = ("none", "both", "tiles", "small")  # form 3 only: atomics / two-pass tiles and bias / tiles only / too small
_TWO_PASS = {"none": 0, "both": 3, "tiles": 1, "small": 0}


@dataclass(frozen=True)
class Case:
    form: int
    dtype: torch.dtype
    scratch: str = "none"

    @property
    def id(self):
        return f"form{self.form}-{DT_NAME[self.dtype]}" + (f"-{self.scratch}" if self.form == 3 else "")

    @property
    def probs(self):
        return BATCHES[self.form]

    @property
    def plan(self):
        p = _PLANS[self.form]
        return Plan(p.form, p.narrow, p.items, _TWO_PASS[self.scratch], p.splits)

    @property
    def scratch_bytes(self):
        """sized from the plan's item count"""
        n = _PLANS[self.form].items
        return {"none": 0, "both": n * (SLOT_BYTES + BIAS_ROW_BYTES), "tiles": n * SLOT_BYTES + BIAS_ROW_BYTES, "small": 1 << 20}[self.scratch]

    @property
    def riders(self):
        """three column-sum jobs and two outer-product jobs travel with the batch: as extra workgroups of the reduction pass
        (both) and as launches of their own (none)"""
        return self.form == 3 and self.scratch in ("none", "both")


CASES = tuple(Case(f, d, s) for d in DTYPES for f in range(4) for s in (SCRATCH_MODES if f == 3 else ("none",)))


def plan_dict(plan):
    """a Plan in the shape ops.gemm_wgrad_plan returns"""
    return dict(form=plan.form, narrow=plan.narrow, items=plan.items, two_pass=plan.two_pass, splits=list(plan.splits))


def tiles(p, form, narrow):
    bn, bk = TILE[form]
    return cdiv(p.N, bn) * cdiv(p.K, 128 if narrow else bk)


def plan_args(probs, dtype, WgradArgs, **over):
    """the problems as mst_wgrad_args with dummy 16-byte-aligned pointers: for mst_gemm_wgrad_plan, which follows none of them.
    over: field -> value, applied to every problem"""
    out = []
    for p in probs:
        w = WgradArgs()
        w.dtype, w.a_u8 = (0 if dtype == BF else 1), int(p.a_u8)
        w.M, w.N, w.K = p.M, p.N, p.K
        w.A, w.lda, w.B, w.ldb, w.dW, w.ldw = 4096, p.lda, 4096, p.ldb, 4096, p.ldw
        w.db = 4096 if p.db else None
        w.scale = p.scale
        w.a_rows_per_group, w.a_group_stride, w.a_group_offset = p.remap(p.ta)
        w.b_rows_per_group, w.b_group_stride, w.b_group_offset = p.remap(p.tb)
        for k, v in over.items():
            setattr(w, k, v)
        out.append(w)
    return out


# ------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(form, dtype, mode):
    """the batch's operands as CPU tensors, deterministic, one dict per problem (shared by the tests: leave them unchanged).
    int mode: A in [-3, 3], B in [-2, 2] — every partial sum is exact in fp32 in any order. real mode: A ~ N(0, 1), B ~ 0.2 N(0, 1),
    rounded to the dtype. uint8 A in both: {0, 1} at density 0.5 with some 2..6. dW0 / db0: the small integers the outputs hold
    before the launch (both are accumulated into). Pad columns up to roundup8 hold zeros (the contract); columns beyond, and the
    physical rows a remap skips, hold NaN: the kernel must never read them."""
    out = []
    for i, p in enumerate(BATCHES[form]):
        g = torch.Generator().manual_seed(7000 + 100 * form + i + (50 if dtype == FP else 0) + (1000 if mode == "real" else 0))

        def mat(rows, cols, ld, t, lo, hi, sigma):
            if mode == "int":
                v = torch.randint(lo, hi + 1, (rows, cols), generator=g).to(dtype)
            else:
                v = (torch.randn((rows, cols), generator=g) * sigma).to(dtype)
            full = torch.full((p.rows(t), ld), float("nan"), dtype=dtype)
            full[:, cols:roundup(cols, 8)] = 0
            full[torch.from_numpy(p.phys(t)), :cols] = v
            if t:
                full[::t + 1, :roundup(cols, 8)] = float("nan")  # the skipped row of every group, pad columns included
            return full

        if p.a_u8:
            assert not p.ta and not p.pad and p.lda == roundup(p.N, 8)
            A = torch.zeros((p.M, p.lda), dtype=torch.uint8)
            A[:, :p.N] = (torch.rand((p.M, p.N), generator=g) < 0.5).to(torch.uint8)
            r, c = torch.arange(0, p.M, 7), torch.arange(0, p.N, 5)
            A[r[:, None], c[None, :]] = (2 + (r[:, None] + c[None, :]) % 5).to(torch.uint8)
        else:
            A = mat(p.M, p.N, p.lda, p.ta, -3, 3, 1.0)
        B = mat(p.M, p.K, p.ldb, p.tb, -2, 2, 0.2)
        dW0 = torch.randint(-2, 3, (p.N, p.K), generator=g).double().numpy()
        db0 = torch.randint(-2, 3, (p.N,), generator=g).double().numpy()
        out.append(dict(A=A, B=B, dW0=dW0, db0=db0))
    return tuple(out)


def gathered(p, o, drop_row=None, a_shift=0, b_shift=0):
    """-> (A [M', N], B [M', K]) fp64: the logical rows through the restated remap. The three mutations the discrimination tests
    use: one logical row left out of the sum, or a remap's offset moved by a row"""
    pa, pb = p.phys(p.ta) + a_shift, p.phys(p.tb) + b_shift
    A = o["A"][torch.from_numpy(pa), :p.N].double().numpy()
    B = o["B"][torch.from_numpy(pb), :p.K].double().numpy()
    if drop_row is not None:
        A, B = np.delete(A, drop_row, axis=0), np.delete(B, drop_row, axis=0)
    return A, B


def wgrad_ref(p, o, **mut):
    """-> dict(dW, SW [N, K], db, Sb [N]) fp64: dW0 + scale A^T B, db0 + scale colsum(A) (db0 where the problem has no bias:
    it must stay), and the same sums on absolute values, what wgrad_bound scales the accumulation error by"""
    A, B = gathered(p, o, **mut)
    s = float(np.float32(p.scale))
    return dict(dW=o["dW0"] + s * (A.T @ B), SW=abs(s) * (np.abs(A).T @ np.abs(B)),
                db=o["db0"] + (s * A.sum(0) if p.db else 0.0), Sb=(abs(s) * np.abs(A).sum(0) if p.db else np.zeros(p.N)))


@functools.lru_cache(maxsize=None)
def references(form, dtype, mode):
    return tuple(wgrad_ref(p, o) for p, o in zip(BATCHES[form], operands(form, dtype, mode)))


def wgrad_bound(M, ref, S):
    """the tolerance of every output element in real mode, derived: one rounding into the accumulated output (2^-24 |ref|), plus the
    standard bound of an fp32 sum of M terms in any order and the few scale and merge operations ((M + 16) 2^-24 S), doubled because
    MFMA accumulation need not round every addition the IEEE way. Independent of the M split and of atomics versus two-pass."""
    return 2.0 ** -24 * np.abs(ref) + 2.0 * (M + 16) * 2.0 ** -24 * S


# ------------------------------------------------------------------------------------------ the rider jobs
SUM_SPECS = ((37, 0, 256), (20, 64, 128), (1, 4, 60))  # (parts, first column, length) of a [37, 256] table of partial rows


@functools.lru_cache(maxsize=None)
def rider_operands(dtype):
    """integer data: the column sums and the outer products are exact"""
    g = torch.Generator().manual_seed(4242)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
    return dict(part=ri(-8, 8, (37, 256)), L0=ri(-3, 3, (8, 24)), R0=ri(-3, 3, (8, 40)), L1=ri(-3, 3, (13, 16)),
                R1=ri(-2, 2, (13, 48)).to(dtype))  # R1: 16-bit rows of stride 48, the first 40 columns used


def rider_refs(r):
    """-> (column sums on top of ones, [out0 [24, 40], out1 [16, 40] on top of ones, obias1 [16] on top of ones])"""
    sums = [1.0 + r["part"][:n, off:off + length].double().sum(0).numpy() for n, off, length in SUM_SPECS]
    L0, R0, L1, R1 = (r[k].double().numpy() for k in ("L0", "R0", "L1", "R1"))
    return sums, [L0.T @ R0, 1.0 + L1.T @ R1[:, :40], 1.0 + L1.sum(0)]
