"""Plain fp64 references of the latent block (csrc/latent.hip, latent_fwd.hpp, outer_jobs.hpp; no GPU, no library), the bounds its
launches are held to, and the table of cases that reaches every launch form (mst_latent_form in include/mst_hip.h).

The operation, per sample b (fp32 math on 16-bit activations; [x]16 is a rounding to the activation type):
    forward    [mu | sigma] = h0 Wl^T + bl             z = mu + eps sigma        kl = 0.5 sum(sigma^2 + mu^2 - 1 - log sigma^2)
               dec = [alpha (z Wh^T + bh + cls[c_b]) + pos]16                    qkv0 = [dec Wq^T + bq]16
    backward   t = alpha g   (read form)   or   t = alpha [dq Wt^T + resid]16   (proj form)
               a = t Wh      dmu = klw gscale mu + enc_scale a      dsigma = klw gscale (sigma - 1 / sigma) + enc_scale eps a
               d_enc = [[dmu | dsigma] Wl]16         dcls[c] += sum of t over the samples of class c, in batch order
    outer      out[j, i] += sum_b L[b, j] R[b, i]    obias[j] += sum_b L[b, j]   (dWl, dbl from [dmu | dsigma] and h0; dWh, dbh from t and z)

References are STAGED: every quantity is computed in fp64 from the inputs the launch itself read, i.e. from the upstream values the
launch stored, so that each bound covers one stage's arithmetic and nothing else. With u = 2^-24:
    dot(n, S)   an fp32 dot product of n terms in any order, fused or not, plus up to two more additions: (n + 2) u S, S = sum |x||w| + |addends|
    h16(x)      half a unit in the last place of the 16-bit type at |x| (a tie may round either way)
The one number that is not pure arithmetic is the logarithm: HIP documents logf at 1 ulp; 2 ulp of |log sigma^2| are granted per term.

Two operand modes. real: unit-scale values, sigma of both signs with 2^-6 <= |sigma| <= 4 (never 0: there is no epsilon in the log).
int: small integers and dyadic fractions built so that mu, sigma, z, the dec row, t, dcls and the outer products are EXACT in fp32 in
any order and fit the 16-bit type without rounding (alpha is a power of two, sigma is +-1 or +-2): they are compared with ==, and a
lost or doubled term cannot hide. Long contractions stay small there by cancellation: the input is built as x[2k+1] = -x[2k] and the
weights as w[2k+1] = w[2k] != 0 except in a few pairs per row, so every single term still moves the result when it is lost."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

BF, FP = torch.bfloat16, torch.float16
DTYPES = (BF, FP)
DT_NAME = {BF: "bf16", FP: "fp16"}
MODES = ("int", "real")
SENTINEL = 7.0
U = 2.0 ** -24
PAD = 8           # pad columns of a strided 16-bit operand (keeps rows 16-byte aligned); fp32 tables take 3
LAT_THREADS = 1024


# ------------------------------------------------------------------------------------------ the launch forms, restated
def fwd_pre_shape(De, Z, Dd):
    """latent_fwd_pre_shape: both products in one pass of 8 outputs per wave (16 waves), weights of 4 chunks of 64 in registers"""
    return 2 * Z <= 128 and De <= 256 and Dd <= 128 and Z <= 64


def bwd_pre_shape(De, Z, Dd):
    """latent_bwd_pre_shape: at most 8 rows of Wh and 32 rows of Wl per thread"""
    if Z > LAT_THREADS or De > LAT_THREADS:
        return False
    np_h, np_l = LAT_THREADS // Z, LAT_THREADS // De
    return -(-Dd // np_h) <= 8 and -(-2 * Z // np_l) <= 32


def fwd_form(De, Z, Dd, nq=0):
    pre = fwd_pre_shape(De, Z, Dd)
    loader = lambda n: 0 if pre else 1 if n <= 256 else 2  # noqa: E731
    return (int(pre), loader(De), loader(Z), (Dd // 64 if nq else 0), 4 * (De + 3 * Z + (Dd + nq if nq else 0)))


def bwd_form(De, Z, Dd, wl_off=0):
    pre = bwd_pre_shape(De, Z, Dd)
    four = De % 4 == 0 and De // 4 <= LAT_THREADS and wl_off % 4 == 0
    return (int(pre), 0 if pre else 1 if four else 2, 4 * (Dd + 2 * Z + (1 if pre else 4) * LAT_THREADS + 4))


# ------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Fwd:
    name: str
    B: int
    De: int
    Z: int
    Dd: int
    ncls: int
    form: tuple            # (preloaded, loader of h0 . Wl, loader of z . Wh, VEC of the projection, LDS bytes): entries 0..4
    nq: int = 0            # outputs of the row-0 projection (0: mst_latent_fwd)
    bq: bool = True
    wq_pad: int = 0        # ld_wq - Dd
    qkv_pad: int = 0       # columns of a qkv row behind nq

    @property
    def id(self):
        return "fwd-" + self.name


@dataclass(frozen=True)
class Bwd:
    name: str
    B: int
    De: int
    Z: int
    Dd: int
    ncls: int
    form: tuple            # (preloaded, dh0 path, LDS bytes): entries 5..7
    nq: int = 0            # columns of the transposed projection weight (0: the read form)
    resid: bool = True
    wt_pad: int = 0        # ld_wt - nq
    wl_off: int = 0        # floats Wl is offset by from a 16-byte boundary
    sched: bool = False    # also run as mst_latent_bwd_vec_sched, bit-identical at kl_weight = beta

    @property
    def id(self):
        return "bwd-" + self.name


FWD = (
    Fwd("pre-limits", 5, 256, 64, 128, 3, (1, 0, 0, 0, 1792)),                 # exactly on all four limits
    Fwd("pre-ragged", 3, 200, 33, 100, 2, (1, 0, 0, 0, 1196)),
    Fwd("z65", 4, 256, 65, 128, 2, (0, 1, 1, 0, 1804)),                        # one step outside each limit; 2Z = 130: a pass of 2
    Fwd("de257", 4, 257, 64, 128, 2, (0, 2, 1, 0, 1796)),
    Fwd("dd129", 4, 256, 64, 129, 2, (0, 1, 1, 0, 1792)),                      # ONE pass of 128 outputs in the first product
    Fwd("z192", 3, 256, 192, 128, 2, (0, 1, 1, 0, 3328)),                      # three passes
    Fwd("z256", 5, 256, 256, 128, 3, (0, 1, 1, 0, 4096)),                      # four passes: the configs[2] shape
    Fwd("ragged", 3, 250, 99, 77, 4, (0, 1, 1, 0, 2188)),                      # 198 outputs: a last pass of 8 waves and 6 outputs
    Fwd("de320", 3, 320, 64, 128, 2, (0, 2, 1, 0, 2048)),                      # wave_dots in the first product
    Fwd("z260", 3, 256, 260, 128, 2, (0, 1, 2, 0, 4144)),                      # ... and in the second
    Fwd("proj64", 4, 256, 64, 64, 2, (1, 0, 0, 1, 2816), nq=192),
    Fwd("proj64-nq200", 3, 200, 33, 64, 2, (1, 0, 0, 1, 2252), nq=200, bq=False),
    Fwd("proj128-pre", 5, 256, 64, 128, 3, (1, 0, 0, 2, 3840), nq=384, wq_pad=PAD),
    Fwd("proj128-general", 3, 256, 256, 128, 2, (0, 1, 1, 2, 6144), nq=384, qkv_pad=PAD),
    Fwd("proj256", 3, 256, 64, 256, 2, (0, 1, 1, 4, 5888), nq=768, wq_pad=PAD, qkv_pad=PAD),
)
BWD = (
    Bwd("pre-limits", 5, 256, 64, 128, 3, (1, 0, 5136), sched=True),
    Bwd("pre-ragged", 3, 200, 33, 100, 2, (1, 0, 4776)),                       # 33 does not divide 1024: thread 1023 owns nothing
    Bwd("four", 4, 256, 256, 128, 3, (0, 1, 18960), sched=True),               # the configs[2] shape
    Bwd("four-short", 2, 1024, 40, 64, 2, (0, 1, 16976)),                      # dz: 3 terms per thread; dh0: 20 = 2.5 batches of 8
    Bwd("scalar-de258", 3, 258, 256, 128, 2, (0, 2, 18960), sched=True),
    Bwd("scalar-offset", 3, 256, 256, 128, 2, (0, 2, 18960), wl_off=1),
    Bwd("scalar-two-rounds", 2, 1030, 40, 64, 2, (0, 2, 16976)),
    Bwd("proj384", 5, 256, 64, 128, 3, (1, 0, 5136), nq=384),
    Bwd("proj384-general", 3, 256, 256, 128, 2, (0, 1, 18960), nq=384, resid=False, wt_pad=PAD),
    Bwd("proj768", 3, 256, 64, 256, 2, (0, 1, 17936), nq=768, resid=False),
    Bwd("proj768-resid", 2, 200, 33, 256, 2, (0, 1, 17688), nq=768, wt_pad=PAD),
    Bwd("z1024", 2, 64, 1024, 32, 2, (0, 1, 24720)),
    # the class table: more than four classes take a second and a third pass; quarters of 16 rows take the chunked loop (B 64), 18
    # rows chunk + tail (B 70)
    Bwd("cls-b1", 1, 64, 16, 100, 1, (1, 0, 4640)),
    Bwd("cls-b3", 3, 64, 16, 128, 2, (1, 0, 4752)),
    Bwd("cls-b5", 5, 64, 16, 100, 5, (1, 0, 4640)),
    Bwd("cls-b64", 64, 64, 16, 128, 9, (1, 0, 4752)),
    Bwd("cls-b70", 70, 64, 16, 100, 9, (1, 0, 4640)),
    Bwd("cls-b70-5", 70, 64, 16, 128, 5, (1, 0, 4752)),
)
CASES = FWD + BWD
# the launch constants: alpha a power of two in int mode (it is an argument); gscale and enc_scale differ from 1 so that a scale
# left off shows. (kl_weight, gscale, enc_scale)
ALPHA = {"int": 2.0, "real": None}  # real: sqrt(Dd), as the model sets it
SCALES = {"int": (0.5, 4.0, 0.5), "real": (0.75, 4.0, 0.5)}


def alpha_of(c, mode):
    return float(np.float32(ALPHA[mode] if ALPHA[mode] else np.sqrt(c.Dd)))


def classes_of(c):
    """every class occurs where B allows; the order is not sorted"""
    return (np.arange(c.B) * 7 + 3) % c.ncls if c.B >= c.ncls else np.arange(c.B) % c.ncls


# ------------------------------------------------------------------------------------------ operands
def r16(x, dtype):
    """fp64 / fp32 values -> the 16-bit type (round to nearest even) -> fp64"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(torch.float32).to(dtype).double().numpy()


def _seed(c, dtype, mode):
    return 9000 + 97 * CASES.index(c) + (31 if dtype == FP else 0) + (5000 if mode == "real" else 0)


def _ri(g, lo, hi, shape, nonzero=False):
    v = torch.randint(lo, hi + 1, shape, generator=g).double().numpy()
    if nonzero:
        v = np.where(v == 0, 1.0, v)
    return v


def _anti(v):
    """x[..., 2k+1] = -x[..., 2k] (an odd tail stays free)"""
    v = v.copy()
    n = v.shape[-1] // 2 * 2
    v[..., 1:n:2] = -v[..., 0:n:2]
    return v


def _cancel_rows(g, rows, n, nfree, tail=True):
    """[rows, n] weights in {-1, 1}: w[2k+1] = w[2k] (cancels against an _anti input) except in nfree pairs per row where
    w[2k+1] = -w[2k]; an odd last column is free (or zero)"""
    W = _ri(g, 0, 1, (rows, n)) * 2 - 1
    m = n // 2 * 2
    W[:, 1:m:2] = W[:, 0:m:2]
    for j in range(rows):
        for k in torch.randperm(max(n // 2, 1), generator=g)[:nfree].tolist():
            if 2 * k + 1 < m:
                W[j, 2 * k + 1] = -W[j, 2 * k]
    if n % 2 and not tail:
        W[:, -1] = 0
    return W


def _rn(g, shape, scale=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float64).numpy() * scale


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def operands(c, dtype, mode):
    """a case's dense operands as fp64 numpy arrays holding values of their storage type (shared by the tests: leave them unchanged)"""
    g = torch.Generator().manual_seed(_seed(c, dtype, mode))
    B, De, Z, Dd = c.B, c.De, c.Z, c.Dd
    o = dict(classes=classes_of(c).astype(np.int64), alpha=alpha_of(c, mode))
    if isinstance(c, Fwd):
        if mode == "int":
            o["h"] = _anti(_ri(g, -2, 2, (B, De), nonzero=True))
            half = _cancel_rows(g, Z, De, 2)
            half[1:Z // 2 * 2:2] = -half[0:Z // 2 * 2:2]            # mu[2k+1] = -mu[2k]
            sg = _cancel_rows(g, Z, De, 0, tail=False)                  # sigma = its bias: +-1 or +-2
            sg[1:Z // 2 * 2:2] = -sg[0:Z // 2 * 2:2]
            o["Wl"] = np.concatenate([half, sg])
            bs = (_ri(g, 1, 2, (Z,))) * (_ri(g, 0, 1, (Z,)) * 2 - 1)
            o["bl"] = np.concatenate([_anti(_ri(g, -1, 1, (Z,))), _anti(bs)])
            e = _ri(g, -2, 2, (B, Z)) / 2
            n = Z // 2 * 2
            e[:, 1:n:2] = e[:, 0:n:2]                                   # so that z[2k+1] = -z[2k]
            o["eps"] = e
            o["Wh"] = _cancel_rows(g, Dd, Z, 1)
            o["bh"], o["cls"], o["pos"] = _ri(g, -1, 1, (Dd,)), _ri(g, -1, 1, (c.ncls, Dd)), _ri(g, -2, 2, (Dd,), nonzero=True)
            if c.nq:
                o["Wq"], o["bq"] = _ri(g, -1, 1, (c.nq, Dd), nonzero=True), _ri(g, -2, 2, (c.nq,))
        else:
            o["h"] = r16(_rn(g, (B, De)), dtype)
            bs = 2.0 ** (torch.rand((Z,), generator=g, dtype=torch.float64).numpy() * 6.5 - 5.0) * (_ri(g, 0, 1, (Z,)) * 2 - 1)
            # sigma = its bias (2^-5 .. 2^1.5, both signs) * (1 + 0.08 N(0, 1)): inside 2^-6 .. 4 at five deviations
            o["Wl"] = f32(np.concatenate([_rn(g, (Z, De), De ** -0.5), _rn(g, (Z, De), 0.08 * De ** -0.5) * np.abs(bs)[:, None]]))
            o["bl"] = f32(np.concatenate([_rn(g, (Z,), 0.5), bs]))
            o["eps"] = f32(_rn(g, (B, Z)))
            o["Wh"], o["bh"] = f32(_rn(g, (Dd, Z), Z ** -0.5)), f32(_rn(g, (Dd,), 0.1))
            o["cls"], o["pos"] = f32(_rn(g, (c.ncls, Dd))), f32(_rn(g, (Dd,)))
            if c.nq:
                o["Wq"], o["bq"] = r16(_rn(g, (c.nq, Dd), Dd ** -0.5), dtype), f32(_rn(g, (c.nq,), 0.2))
        if c.nq and not c.bq:
            o["bq"] = np.zeros(c.nq)
    else:
        o["klw"], o["gscale"], o["enc_scale"] = SCALES[mode]
        if mode == "int":
            o["mu"], o["eps"] = _ri(g, -3, 3, (B, Z)), _ri(g, -2, 2, (B, Z)) / 2
            o["sigma"] = _ri(g, 1, 2, (B, Z)) * (_ri(g, 0, 1, (B, Z)) * 2 - 1)
            o["Wl"], o["Wh"] = _ri(g, -2, 2, (2 * Z, De)), _ri(g, -2, 2, (Dd, Z))
            o["g"] = _ri(g, -3, 3, (B, Dd), nonzero=True)
            o["dq"], o["Wt"] = _anti(_ri(g, -2, 2, (B, max(c.nq, 2)), nonzero=True)), _cancel_rows(g, Dd, max(c.nq, 2), 2)
            o["resid"] = _ri(g, -2, 2, (B, Dd))
            o["dcls0"] = _ri(g, -2, 2, (c.ncls, Dd), nonzero=True)
            o["h"], o["z"] = _ri(g, -2, 2, (B, De)), _ri(g, -4, 4, (B, Z)) / 2
            o["out0"] = [_ri(g, -2, 2, s, nonzero=True) for s in ((2 * Z, De), (2 * Z,), (Dd, Z), (Dd,))]
        else:
            o["mu"], o["eps"] = f32(_rn(g, (B, Z))), f32(_rn(g, (B, Z)))
            o["sigma"] = f32(2.0 ** (torch.rand((B, Z), generator=g, dtype=torch.float64).numpy() * 8 - 6) * (_ri(g, 0, 1, (B, Z)) * 2 - 1))
            o["Wl"], o["Wh"] = f32(_rn(g, (2 * Z, De), De ** -0.5)), f32(_rn(g, (Dd, Z), Z ** -0.5))
            o["g"] = r16(_rn(g, (B, Dd), 0.3), dtype)
            o["dq"], o["Wt"] = r16(_rn(g, (B, max(c.nq, 2)), 0.3), dtype), r16(_rn(g, (Dd, max(c.nq, 2)), max(c.nq, 2) ** -0.5), dtype)
            o["resid"] = r16(_rn(g, (B, Dd), 0.3), dtype)
            o["dcls0"] = f32(_rn(g, (c.ncls, Dd)))
            o["h"], o["z"] = r16(_rn(g, (B, De)), dtype), f32(_rn(g, (B, Z)))
            o["out0"] = [f32(_rn(g, s)) for s in ((2 * Z, De), (2 * Z,), (Dd, Z), (Dd,))]
        if c.nq and not c.resid:
            o["resid"] = np.zeros((B, Dd))
    return o


# ------------------------------------------------------------------------------------------ arithmetic in a chosen precision
def _sum(p, order):
    """the last axis summed in p's own precision: one after the other, or pairwise (the two orders furthest apart)"""
    if p.dtype == np.float64 or p.shape[-1] == 0:
        return p.sum(-1)
    if order == "seq":
        return np.cumsum(p, axis=-1, dtype=p.dtype)[..., -1]
    while p.shape[-1] > 1:
        if p.shape[-1] % 2:
            p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), p.dtype)], -1)
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def dot(x, W, prec, order="seq", mut=None):
    """x [B, n] . W [J, n] -> [B, J] in prec. mut: drop_last / double_first, the two wrong dot products of a pipelined loader"""
    if mut == "drop_last":
        x, W = x[:, :-1], W[:, :-1]
    elif mut == "double_first":
        x, W = np.concatenate([x[:, :1], x], 1), np.concatenate([W[:, :1], W], 1)
    x, W = x.astype(prec), W.astype(prec)
    if prec == np.float64:
        return x @ W.T
    return _sum(x[:, None, :] * W[None, :, :], order)


def absdot(x, W):
    return np.abs(x) @ np.abs(W).T


def h16(x, dtype):
    """half a unit in the last place of the 16-bit type at |x| (8 / 11 significant bits; fp16's subnormals below 2^-14)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 1e-300)))
    return 2.0 ** (np.maximum(e, -126.0) - 8) if dtype == BF else 2.0 ** (np.maximum(e, -14.0) - 11)


def _m(mut, site):
    """the dot-product mutation `kind@site` where it is this site's"""
    return mut.split("@")[0] if mut and mut.endswith("@" + site) else None


# ------------------------------------------------------------------------------------------ the forward pass
def run_fwd(c, o, dtype, prec=np.float32, order="seq", mut=None):
    """every stored quantity of the forward launch, each stage computed in prec from the stage before AS STORED -> dict of fp64
    arrays. prec = float32: the emulation the bounds must accept; mut: one wrong kernel (tests/test_latent_refs_cpu.py)"""
    P = prec
    a = P(o["alpha"])
    lat = (dot(o["h"], o["Wl"], P, order, _m(mut, "lat")) + o["bl"].astype(P)).astype(P)
    mu, sg = lat[:, :c.Z], lat[:, c.Z:]
    eps = (np.roll(o["eps"], -1, 0) if mut == "eps_next" else o["eps"]).astype(P)
    z = mu + eps * sg
    s2 = sg * sg
    with np.errstate(divide="ignore", invalid="ignore"):  # (a wrong kernel's sigma may be 0: its kl is then inf, and refused)
        term = P(0.5) * (s2 + mu * mu - (P(0) if mut == "kl_no_minus1" else P(1)) - np.log(s2))
    kl = _sum(term[:, :-1] if mut == "kl_drop_last" else term, order)
    inner = dot(z, o["Wh"], P, order, _m(mut, "dec")) + o["bh"].astype(P) + o["cls"][o["classes"]].astype(P)
    pos = o["pos"].astype(P)
    dec = r16(a * inner + (a * pos if mut == "pos_scaled" else pos), dtype)
    out = dict(mu=mu, sigma=sg, z=z, kl=kl, dec=dec)
    if c.nq:
        out["qkv"] = r16(dot(dec, o["Wq"], P, order, _m(mut, "qkv")) + o["bq"].astype(P), dtype)
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def fwd_refs(c, o, dtype, got):
    """-> {quantity: (reference, bound)} for what a launch stored (got: run_fwd's dict), staged"""
    De, Z, Dd = c.De, c.Z, c.Dd
    a = o["alpha"]
    res = {}
    lat, S = o["h"] @ o["Wl"].T + o["bl"], absdot(o["h"], o["Wl"]) + np.abs(o["bl"])
    b = (De + 2) * U * S
    res["mu"], res["sigma"] = (lat[:, :Z], b[:, :Z]), (lat[:, Z:], b[:, Z:])
    m, s = got["mu"], got["sigma"]
    z = m + o["eps"] * s
    res["z"] = (z, U * (np.abs(o["eps"] * s) + np.abs(z)) * (1 + 2.0 ** -20))                      # two roundings
    # kl: per term at most four roundings of values below A = s^2 + m^2 + 1 + |log s^2| (five unfused ones stay below 4 u A too), the
    # rounding of s^2 moves the logarithm by at most u, logf itself 2 ulp; then a Z-term fp32 sum in any order
    s2 = s * s
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.log(s2)
        term = 0.5 * (s2 + m * m - 1 - L)
    A = s2 + m * m + 1 + np.abs(L)
    ulp_log = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(L), 2.0 ** -126))) - 23)
    terr = 0.5 * (4 * U * A + U + 2 * ulp_log)
    res["kl"] = (term.sum(1), terr.sum(1) + Z * U * (np.abs(term) + terr).sum(1))
    zz = got["z"]
    cls = o["cls"][o["classes"]]
    inner = zz @ o["Wh"].T + o["bh"] + cls
    S = absdot(zz, o["Wh"]) + np.abs(o["bh"]) + np.abs(cls)
    x = a * inner + o["pos"]
    e32 = (Z + 2) * U * a * S + U * (a * np.abs(inner) + np.abs(x))                               # the dot, the alpha and the pos roundings
    res["dec"] = (x, e32 + h16(np.abs(x) + e32, dtype))
    if c.nq:
        d = got["dec"]
        q = d @ o["Wq"].T + o["bq"]
        e32 = (Dd + 2) * U * (absdot(d, o["Wq"]) + np.abs(o["bq"]))
        res["qkv"] = (q, e32 + h16(np.abs(q) + e32, dtype))
    return res


FWD_EXACT = ("mu", "sigma", "z", "dec")  # int mode: compared with ==


# ------------------------------------------------------------------------------------------ the backward pass
def class_table(t, classes, dcls0, prec, order="seq", mut=None):
    out = dcls0.astype(prec).copy()
    for k in range(dcls0.shape[0]):
        rows = t[(classes == k) | ((classes == k + 4) if mut == "cls_plus4" else False)].astype(prec)
        if len(rows):
            out[k] = out[k] + _sum(rows.T, order)
    return out


def outer(L, R, out0, bias0, prec, order="seq", mut=None):
    """-> (out0 + L^T R, bias0 + column sums of L). mut outer_skip: the last sample of the first quarter of the batch left out"""
    if mut == "outer_skip":
        keep = np.arange(L.shape[0]) != (L.shape[0] + 3) // 4 - 1
        L, R = L[keep], R[keep]
    out = out0.astype(prec) + dot(L.T, R.T, prec, order)
    return out, (None if bias0 is None else bias0.astype(prec) + _sum(L.T.astype(prec), order))


def run_bwd(c, o, dtype, prec=np.float32, order="seq", mut=None):
    P = prec
    a, klw, gs, es = P(o["alpha"]), P(o["klw"]), P(o["gscale"]), P(o["enc_scale"])
    if c.nq:
        v = dot(o["dq"], o["Wt"], P, order, _m(mut, "tproj")) + o["resid"].astype(P)
        t = a * (v if mut == "t_unrounded" else r16(v, dtype).astype(P))
    else:
        t = a * o["g"].astype(P)
    acc = dot(t, o["Wh"].T, P, order, _m(mut, "dz"))
    m, s = o["mu"].astype(P), o["sigma"].astype(P)
    e = (np.roll(o["eps"], -1, 0) if mut == "eps_next" else o["eps"]).astype(P)
    kg = klw if mut == "no_gscale" else klw * gs
    es = P(1) if mut == "no_enc_scale" else es
    inv = P(1) / s
    dlat = np.concatenate([kg * m + es * acc, kg * ((s + inv) if mut == "s_plus_inv" else (s - inv)) + es * e * acc], 1)
    denc = r16(dot(dlat, o["Wl"].T, P, order, _m(mut, "dh0")), dtype)
    out = dict(t=t, dlat=dlat, denc=denc, dcls=class_table(t, o["classes"], o["dcls0"], P, order, mut))
    out["dWl"], out["dbl"] = outer(dlat, o["h"], o["out0"][0], o["out0"][1], P, order, mut)
    out["dWh"], out["dbh"] = outer(t, o["z"], o["out0"][2], o["out0"][3], P, order, mut)
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def outer_refs(L, R, out0, bias0):
    """-> ((out, bound), (bias, bound)): a B-term dot and the rounding into the accumulated output"""
    B = L.shape[0]
    out = (out0 + L.T @ R, (B + 2) * U * (np.abs(out0) + np.abs(L).T @ np.abs(R)))
    return out, (None if bias0 is None else (bias0 + L.sum(0), (B + 2) * U * (np.abs(bias0) + np.abs(L).sum(0))))


def bwd_refs(c, o, dtype, got, exact_sigma=False):
    """-> {quantity: (reference, bound)}, staged. exact_sigma (int mode): dlat has no rounding where |sigma| = 1 (s - 1 / s = 0) and in
    dmu; where sigma = +-2 the division's bound stays"""
    Z, Dd = c.Z, c.Dd
    a, klw, gs, es = o["alpha"], f32(o["klw"]), f32(o["gscale"]), f32(o["enc_scale"])
    res = {}
    if c.nq:
        v = o["dq"] @ o["Wt"].T + o["resid"]
        e32 = (c.nq + 2) * U * (absdot(o["dq"], o["Wt"]) + np.abs(o["resid"]))
        res["t"] = (a * v, a * (e32 + h16(np.abs(v) + e32, dtype)) + U * a * (np.abs(v) + e32))
        # ... and WHERE the 16-bit rounding sits: the stored t is alpha times a 16-bit value, exactly (alpha has 24 bits, the value 11
        # or 8: the product has one rounding, and dividing it out lands within u of the 16-bit value it came from)
        res["t16"] = (f32(a * r16(got["t"] / a, dtype)), np.zeros_like(v))
    else:
        t = a * o["g"]
        res["t"] = (t, U * np.abs(t))
    t = got["t"]
    acc, Ea = t @ o["Wh"], (Dd + 2) * U * (np.abs(t) @ np.abs(o["Wh"]))
    m, s, e = o["mu"], o["sigma"], o["eps"]
    kg = float(f32(klw * gs))
    dm, ds = kg * m + es * acc, kg * (s - 1 / s) + es * e * acc
    bm = es * Ea + 4 * U * (np.abs(kg * m) + np.abs(es * acc))
    bs = np.abs(kg) * U * (1 / np.abs(s) + 3 * np.abs(s - 1 / s)) + np.abs(es * e) * (Ea + 3 * U * np.abs(acc)) + U * np.abs(ds)
    if exact_sigma:
        bm, bs = np.zeros_like(bm), np.where(np.abs(s) == 1, 0.0, bs)
    res["dlat"] = (np.concatenate([dm, ds], 1), np.concatenate([bm, bs], 1))
    dl = got["dlat"]
    d = dl @ o["Wl"]
    e32 = (2 * Z + 2) * U * (np.abs(dl) @ np.abs(o["Wl"]))
    res["denc"] = (d, e32 + h16(np.abs(d) + e32, dtype))
    ref = class_table(t, o["classes"], o["dcls0"], np.float64)
    S = class_table(np.abs(t), o["classes"], np.abs(o["dcls0"]), np.float64)
    n = np.bincount(o["classes"], minlength=c.ncls)[:, None]
    res["dcls"] = (ref, (n + 4) * U * S)                           # n rows in quarters, the four quarters, the add into the table
    (res["dWl"], res["dbl"]) = outer_refs(dl, o["h"], o["out0"][0], o["out0"][1])
    (res["dWh"], res["dbh"]) = outer_refs(t, o["z"], o["out0"][2], o["out0"][3])
    return res


BWD_EXACT = ("t", "dcls", "dWl", "dbl", "dWh", "dbh")  # int mode: compared with == (dlat: where bwd_refs says so)


def refs_of(c, o, dtype, got, mode):
    return fwd_refs(c, o, dtype, got) if isinstance(c, Fwd) else bwd_refs(c, o, dtype, got, exact_sigma=(mode == "int"))


def run(c, o, dtype, **kw):
    return run_fwd(c, o, dtype, **kw) if isinstance(c, Fwd) else run_bwd(c, o, dtype, **kw)


def judge(c, o, dtype, mode, got):
    """what a launch stored against the staged references -> {quantity: (elements outside the bound, worst error / bound, message)}.
    int mode: the exact quantities must be equal; the others keep their bound."""
    exact = (FWD_EXACT if isinstance(c, Fwd) else BWD_EXACT) if mode == "int" else ()
    out = {}
    for k, (ref, bound) in refs_of(c, o, dtype, got, mode).items():
        g = got["t" if k == "t16" else k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        if k in exact:
            bound = np.zeros_like(ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.abs(g - ref)
            bad = ~(err <= bound)                                  # (a NaN or an infinity anywhere is outside)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        msg = ""
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, np.nan_to_num(ratio, nan=np.inf, posinf=1e300), -1.0)), err.shape)
            msg = (f"{c.id} {DT_NAME[dtype]} {mode}: {int(bad.sum())}/{bad.size} elements of {k} outside the bound; worst at {tuple(int(x) for x in i)}: "
                   f"got {g[i]!r}, want {ref[i]!r}, bound {bound[i]:.3g}")
        out[k] = (int(bad.sum()), float(np.max(np.nan_to_num(ratio, nan=np.inf))) if ratio.size else 0.0, msg)
    return out


# ------------------------------------------------------------------------------------------ outer products on their own
@dataclass(frozen=True)
class Job:
    B: int
    J: int
    I: int                 # noqa: E741
    r: str                 # R's type: f32, bf16 or fp16
    r_pad: int = 0         # r_stride - I
    bias: bool = True


# one entry per launch: one or two jobs. J * I: 35, 960 (a multiple of 64), 117, 357, 2046, 1170
OUTER = (
    (Job(1, 5, 7, "f32"),),
    (Job(3, 24, 40, "bf16", r_pad=8), Job(5, 13, 9, "f32", r_pad=3, bias=False)),
    (Job(33, 17, 21, "fp16", r_pad=3),),
    (Job(70, 66, 31, "bf16", r_pad=9), Job(70, 9, 130, "fp16", r_pad=6)),   # also as riders of a weight-gradient flush
)
R_DTYPE = {"f32": torch.float32, "bf16": BF, "fp16": FP}


@functools.lru_cache(maxsize=None)
def outer_operands(mode):
    """[[dict(L, R, out0, bias0)]] per launch and job, fp64 arrays of storage-type values"""
    g = torch.Generator().manual_seed(777 + (mode == "real"))
    res = []
    for launch in OUTER:
        jobs = []
        for q in launch:
            if mode == "int":
                L, R = _ri(g, -6, 6, (q.B, q.J)) / 4, _ri(g, -3, 3, (q.B, q.I))
                out0, b0 = _ri(g, -2, 2, (q.J, q.I), nonzero=True), _ri(g, -2, 2, (q.J,), nonzero=True)
            else:
                L, R = f32(_rn(g, (q.B, q.J))), _rn(g, (q.B, q.I))
                R = f32(R) if q.r == "f32" else r16(R, R_DTYPE[q.r])
                out0, b0 = f32(_rn(g, (q.J, q.I))), f32(_rn(g, (q.J,)))
            jobs.append(dict(L=L, R=R, out0=out0, bias0=b0 if q.bias else None))
        res.append(jobs)
    return res
