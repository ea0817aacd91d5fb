"""A plain fp64 reference of mst_gemm_nt (no GPU, no library), the tolerance it is held to, and the table of cases that reaches
every kernel form the launch can take (mst_gemm_nt_form in include/mst_hip.h: tile * 16 + variant).

The operation (include/mst_hip.h, mst_gemm_args), on the 16-bit-rounded operands:
    t = alpha * (A B^T + bias + grpadd[grp_index[m / period]]) -> ReLU -> u = dropout(t) [self_resid: u += t]
      -> + rowadd[m % period] -> + resid -> zero where gate <= 0
with A rows and C rows optionally remapped (logical row m at physical row (m / rpg) * stride + offset + m % rpg), the residual at the
logical or (resid_phys) the physical row, and the dropout decision of an element taken at counter (physical C row) * N + column.

The dropout decision is restated here from csrc/common.hpp (dropout_key, dropout_word and the 16-bit fields) in wrapping integer
arithmetic: tests that use keep_mask do not trust the library's own mask kernel."""
from dataclasses import dataclass

import numpy as np
import torch

BF, FP = torch.bfloat16, torch.float16
DTYPES = (BF, FP)
DT_NAME = {BF: "bf16", FP: "fp16"}
SENTINEL = 7.0
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def roundup(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------ the keep decision
def dropout_thr(p):
    """floor(p * 65536) of the fp32 number the kernel is handed (the product is exact: a power of two)"""
    return int(np.float32(p) * np.float32(65536.0))


def dropout_key(seed, site):
    k = ((seed ^ ((0x9E3779B97F4A7C15 * ((site + 1) & _M32)) & _M64)) * 0xD6E8FEB86659FD93) & _M64
    return ((k >> 32) ^ k) & _M32


def dropout_words(key, idx2):
    """dropout_word for an array of 64-bit word indices -> uint32 array"""
    idx2 = np.asarray(idx2, dtype=np.uint64)
    lo = (idx2 & np.uint64(_M32)).astype(np.uint32)
    hi = (idx2 >> np.uint64(32)).astype(np.uint32)
    x = (lo * np.uint32(0x9E3779B1)) ^ np.uint32(key) ^ (hi * np.uint32(0x85EBCA6B))
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    return x


def keep_mask(seed, site, idx, p):
    """-> (keep bool array like idx, scale): element idx uses field idx & 1 of word idx >> 1; kept iff the field is at least
    thr = floor(p * 65536); the inverted-dropout scale is 65536 / (65536 - thr)"""
    idx = np.asarray(idx, dtype=np.uint64)
    thr = dropout_thr(p)
    x = dropout_words(dropout_key(seed & _M64, site & _M32), idx >> np.uint64(1))
    field = np.where((idx & np.uint64(1)).astype(bool), x >> np.uint32(16), x & np.uint32(0xFFFF))
    return field >= np.uint32(thr), 65536.0 / (65536.0 - thr)


# ------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    code: int            # the form this case is meant for: tile * 16 + variant
    dtype: torch.dtype   # activation type
    M: int
    N: int
    K: int
    ldc: int
    c_f32: bool = False
    a_u8: bool = False
    T: int = 0           # row ops: rowadd period = rows per remap group; A and C rows are rows 1..T of every T + 1 (0: no row ops)
    p: float = 0.0
    self_resid: bool = False
    resid_phys: bool = False
    tag: str = ""

    @property
    def id(self):
        return f"tile{self.code >> 4}-v{self.code & 15}-{DT_NAME[self.dtype]}" + (f"-{self.tag}" if self.tag else "")


ALPHA = float(np.float32(1.7))
SEED, SEED_WORD, SITE = 0x0123456789ABCDEF, 0xF00DFACE5EED1234, 3
ALL_CODES = tuple(t * 16 + v for t in range(3) for v in range(10)) + (48,)


def _cases():
    out = []
    # per tile form: (fast M, N, K, T) whole tiles / whole groups, (general M, N without dropout, N with dropout, K, T) ragged
    shapes = {
        0: dict(fast=(128, 128, 64, 64), gen=(150, 70, 72, 72, 50)),        # 64 x 64 tiles, 64-deep: 2 x 2 tiles / 3 x 2 ragged
        1: dict(fast=(64, 128, 512, 64), gen=(50, 70, 72, 512, 25)),        # M <= 64, K = 512: 256-deep stages (K % 256 == 0 is the form's condition)
        2: dict(fast=(6144, 1024, 64, 128), gen=(6100, 998, 1000, 72, 100)),  # 48 x 8 = 384 tiles of 128 x 128; 6100 % 64 != 0: not ragged128
    }
    for dtype in DTYPES:
        for tile, s in shapes.items():
            Mf, Nf, Kf, Tf = s["fast"]
            Mg, Ng, Ngd, Kg, Tg = s["gen"]
            c = tile * 16

            def gen(variant, drop, **kw):
                n = Ngd if drop else Ng
                # ldc > roundup4(N): 8 more columns without dropout (ldc % 8 == 0 for N = 70: interior tiles keep 16-byte stores),
                # 4 more with (ldc % 8 != 0: every tile takes the guarded stores)
                return Case(c + variant, dtype, Mg, n, Kg, roundup(n, 4) + (4 if drop else 8), p=0.2 if drop else 0.0,
                            tag="drop" if drop else "", **kw)

            out += [
                Case(c + 0, dtype, Mf, Nf, Kf, Nf),
                Case(c + 1, dtype, Mf, Nf, Kf, Nf, p=0.2),
                Case(c + 1, dtype, Mf, Nf, Kf, Nf, p=0.5, self_resid=True, tag="self"),
                gen(2, False), gen(2, True),
                gen(3, False, c_f32=True), gen(3, True, c_f32=True),
                Case(c + 4, dtype, Mf, Nf, Kf, Nf + 8, T=Tf, resid_phys=True),
                Case(c + 5, dtype, Mf, Nf, Kf, Nf, T=Tf, p=0.2),
                gen(6, False, T=Tg), gen(6, True, T=Tg, resid_phys=True),
                gen(7, False, T=Tg, c_f32=True, resid_phys=True), gen(7, True, T=Tg, c_f32=True),
                Case(c + 8, dtype, Mf, Nf, Kf, Nf, T=Tf, a_u8=True),
                Case(c + 9, dtype, Mg, Ng, Kg, roundup(Ng, 4) + 8, T=Tg, a_u8=True, resid_phys=True),
            ]
        # three per CU: 57 x 9 = 513 tiles of 128 x 128, the lower edge of 513..768; K = 96 is three 32-deep stages
        out.append(Case(48, dtype, 7296, 1152, 96, 1152))
    return tuple(out)


CASES = _cases()


def layout(c):
    """row counts and leading dimensions of every operand of a case (elements)"""
    G = c.M // c.T if c.T else 0
    assert not c.T or c.M % c.T == 0
    phys = G * (c.T + 1) if c.T else c.M
    ldx = roundup(c.N, 4)
    return dict(A_rows=phys, lda=c.K, ldb=c.K, C_rows=phys, ldc=c.ldc, R_rows=phys if (c.T and c.resid_phys) else c.M, ldr=ldx, ldg=ldx,
                ldra=c.N, ldga=c.N, G=G)


def phys_rows(c):
    """physical row of every logical row (the A and the C remap of a case are the same map)"""
    m = np.arange(c.M, dtype=np.int64)
    return (m // c.T) * (c.T + 1) + 1 + m % c.T if c.T else m


def operands(c):
    """the case's operands as CPU tensors, deterministic; scaled so that fp16 outputs stay far below 65504"""
    L = layout(c)
    g = torch.Generator().manual_seed(1000 + c.code * 2 + (c.dtype == FP))

    def rn(shape, scale, dtype):
        return (torch.randn(shape, generator=g) * scale).to(dtype)

    o = {}
    if c.a_u8:
        o["A"] = (torch.rand((L["A_rows"], c.K), generator=g) < 0.1).to(torch.uint8)
        o["A"][::7, ::5] = 3  # values other than {0, 1}
    else:
        o["A"] = rn((L["A_rows"], c.K), 1.0, c.dtype)
    o["B"] = rn((c.N, c.K), 0.2, c.dtype)
    o["bias"] = rn((c.N,), 1.0, torch.float32)
    o["resid"] = rn((L["R_rows"], L["ldr"]), 1.0, c.dtype)
    o["gate"] = rn((c.M, L["ldg"]), 1.0, c.dtype)
    if c.T:
        o["rowadd"] = rn((c.T, c.N), 1.0, torch.float32)
        o["grpadd"] = rn((3, c.N), 1.0, torch.float32)
        o["grp_index"] = torch.randint(0, 3, (L["G"],), generator=g).to(torch.int32)
    if c.p > 0:
        o["seed_word"] = torch.tensor([SEED_WORD - (1 << 64)], dtype=torch.int64)  # the 64-bit pattern of SEED_WORD
    return o


def call_kwargs(c, o):
    """keyword arguments of ops.gemm_nt / ops.gemm_nt_form for a case (o: its operands, on the device for a launch)"""
    kw = dict(M=c.M, N=c.N, K=c.K, bias=o["bias"], resid=o["resid"], gate=o["gate"], act=1, alpha=ALPHA, resid_phys=c.resid_phys,
              dropout_p=c.p, dropout_seed=SEED, dropout_site=SITE, self_resid=c.self_resid, dropout_seed_ptr=o.get("seed_word"))
    if c.T:
        kw.update(rowadd=o["rowadd"], rowadd_period=c.T, grpadd=o["grpadd"], grp_index=o["grp_index"], a_remap=(c.T, c.T + 1, 1),
                  c_remap=(c.T, c.T + 1, 1))
    return kw


def form_args(c, GemmArgs, **over):
    """the case as an mst_gemm_args with dummy 16-byte-aligned pointers: for mst_gemm_nt_form, which follows none of them"""
    L, P = layout(c), 4096
    g = GemmArgs()
    g.dtype, g.c_f32, g.a_u8 = (0 if c.dtype == BF else 1), int(c.c_f32), int(c.a_u8)
    g.M, g.N, g.K = c.M, c.N, c.K
    g.A, g.lda, g.B, g.ldb, g.C, g.ldc = P, L["lda"], P, L["ldb"], P, L["ldc"]
    g.bias, g.resid, g.ldr, g.gate, g.ldg = P, P, L["ldr"], P, L["ldg"]
    g.act, g.alpha = 1, ALPHA
    if c.T:
        g.rowadd, g.ldra, g.rowadd_period, g.grpadd, g.ldga, g.grp_index = P, L["ldra"], c.T, P, L["ldga"], P
        g.a_rows_per_group, g.a_group_stride, g.a_group_offset = c.T, c.T + 1, 1
        g.c_rows_per_group, g.c_group_stride, g.c_group_offset = c.T, c.T + 1, 1
    g.dropout_p, g.dropout_seed, g.dropout_site, g.self_resid = c.p, SEED, SITE, int(c.self_resid)
    g.dropout_seed_ptr = P if c.p > 0 else None
    g.resid_phys = int(c.resid_phys)
    for k, v in over.items():
        setattr(g, k, v)
    return g


# ------------------------------------------------------------------------------------------ reference and bound
def gemm_ref(c, o):
    """-> (ref, S), fp64 [M, N]: the epilogue in the header's order on the 16-bit-rounded operands, and the same epilogue on
    absolute values (what gemm_bound scales the accumulation error by)"""
    pm = phys_rows(c)
    A = o["A"][torch.from_numpy(pm)].double().numpy()
    B = o["B"].double().numpy()
    N = c.N
    alpha = float(np.float32(ALPHA))
    t, s = A @ B.T, np.abs(A) @ np.abs(B).T
    bias = o["bias"].double().numpy()
    t += bias
    s += np.abs(bias)
    m = np.arange(c.M)
    if c.T:
        ga = o["grpadd"].double().numpy()[o["grp_index"].numpy()[m // c.T]]
        t += ga
        s += np.abs(ga)
    t *= alpha
    s *= abs(alpha)
    np.maximum(t, 0.0, out=t)  # (S keeps the bound of the value before the ReLU: it only shrinks magnitudes)
    if c.p > 0 or c.self_resid:
        if c.p > 0:
            idx = pm.astype(np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
            keep, scale = keep_mask(SEED ^ SEED_WORD, SITE, idx, c.p)
            k = keep * scale
        else:
            k = 1.0
        t, s = (t + t * k, s + s * k) if c.self_resid else (t * k, s * k)
    if c.T:
        ra = o["rowadd"].double().numpy()[m % c.T]
        t += ra
        s += np.abs(ra)
    r = o["resid"][torch.from_numpy(pm if (c.T and c.resid_phys) else m), :N].double().numpy()
    t += r
    s += np.abs(r)
    open_ = o["gate"][:, :N].double().numpy() > 0
    return np.where(open_, t, 0.0), np.where(open_, s, 0.0)


def gemm_bound(c, ref, S):
    """the tolerance of every output element, derived: one rounding at the store (u_out |ref|), plus the standard bound of a
    length-K fp32 sum in any order and the epilogue's few fp32 operations ((K + 16) 2^-24 S), doubled because MFMA accumulation need
    not round every addition the IEEE way, carried through the store's rounding (1 + u_out); fp16 stores may land on a subnormal
    (half a spacing of 2^-24)"""
    u_out = 0.0 if c.c_f32 else (2.0 ** -8 if c.dtype == BF else 2.0 ** -11)
    floor = 2.0 ** -25 if (c.dtype == FP and not c.c_f32) else 0.0
    return u_out * np.abs(ref) + 2.0 * (c.K + 16) * 2.0 ** -24 * S * (1.0 + u_out) + floor
