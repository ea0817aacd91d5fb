"""The reference of tests/rowblock_refs.py, checked without a GPU: it equals torch autograd in fp64, its derived bounds take an fp32
evaluation of every stage in another summation order and refuse each of a list of wrong results on a stated share of the elements
they touch, and the case table reaches the kernels and the hard rows it is meant for."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowblock_refs as R  # noqa: E402

F32 = np.float32
IDS = [c.id for c in R.CASES]


def case(cid):
    return R.CASES[IDS.index(cid)]


# ------------------------------------------------------------------------------------------ an fp32 evaluation of a launch
def _round(x32, dtype):
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).to(dtype).float().numpy()


def emulate(c, ins, wrong=None):
    """the launch in fp32 numpy, every stored tensor rounded to the activation type before the next stage reads it, in another
    summation order than any kernel's: K reversed, the hidden chunks rotated, numpy's pairwise row sums, the parameter gradients
    as per-part sums added up afterwards. wrong: one of the mistakes the bounds must refuse. -> the output buffers
    Two of the mistakes are stand-ins for what a wrong kernel would read: `dgamma_row_twice` counts the LAST OWNED row twice in the
    parameter gradients (a kernel that sums one row too many reads a row behind M - 1, whose contents no buffer here defines);
    `resid_phys` takes the logical-row residual at index (physical row) mod M — the wrap-around only keeps the index inside the
    M-row buffer; what matters is that every row gets another row's residual."""
    bufs, stages = R.plan(c)
    outs = R.outputs(c)
    pm, _ = R.rows(c)
    unrounded = {}
    for name, b in bufs.items():
        if b.free:  # the loss launch's logit gradient, which no stage here computes: any 16-bit values do for the stages behind it
            g = torch.Generator().manual_seed(5)
            R.scatter(c, b, outs[name], _round((torch.randn((c.M, b.width), generator=g) * 0.01).numpy(), c.dtype))

    def val(name):
        return R.gather(c, bufs[name], outs[name] if bufs[name].out else ins[name]).astype(F32)

    def put(name, v):
        R.scatter(c, bufs[name], outs[name], v)

    def gemm(s, unstored=False):
        A, B = val(s.A), val(s.B)
        K, w = A.shape[1], c.D
        if K > w and K % w == 0:
            acc = np.zeros((A.shape[0], B.shape[0]), dtype=F32)
            for ch in list(range(1, K // w)) + [0]:
                sl = slice(ch * w, (ch + 1) * w)
                acc += A[:, sl][:, ::-1] @ B[:, sl][:, ::-1].T
        else:
            acc = A[:, ::-1] @ B[:, ::-1].T
        t = acc
        if s.bias:
            t = t + val(s.bias)
        t = t * F32(s.alpha)
        if s.relu:
            t = np.maximum(t, F32(0))
        if s.p > 0 or s.self_resid:
            counter = np.arange(c.M) if wrong == "logical_counter" else None
            k = R.keep_scale(c, B.shape[0], s.p, s.site, counter).astype(F32) if s.p > 0 else F32(1)
            t = t + t * k if s.self_resid else t * k
        if s.resid:
            r = val(s.resid)
            if wrong == "resid_phys" and unstored:
                r = R.gather(c, bufs[s.resid], ins[s.resid]).astype(F32)[pm % c.M]
            t = t + r
        if s.gate:
            t = np.where(val(s.gate) > 0, t, F32(0))
        return t.astype(F32)

    for s in stages:
        if isinstance(s, R.Gemm):
            t = gemm(s)
            unrounded[s.out] = t
            put(s.out, _round(t, c.dtype))
        elif isinstance(s, R.LnFwd):
            h = val(s.h)
            hs = unrounded[s.h] if (wrong == "unrounded_stats" and s.h in unrounded) else h
            n = F32(h.shape[1])
            eps = F32(1e-6) if wrong == "eps_1e-6" else F32(1e-5)
            mean = hs.sum(1, dtype=F32) / n
            d = hs - mean[:, None]
            if wrong == "one_pass_var":
                var = (hs * hs).sum(1, dtype=F32) / n - mean * mean
            elif wrong == "unbiased_var":
                var = (d * d).sum(1, dtype=F32) / (n - F32(1))
            else:
                var = (d * d).sum(1, dtype=F32) / n
            with np.errstate(invalid="ignore"):
                rstd = F32(1) / (np.sqrt(var) + eps) if wrong == "eps_outside_root" else F32(1) / np.sqrt(var + eps)
            y = (h - mean[:, None]) * rstd[:, None] * val(s.gamma) + val(s.beta)
            put(s.mean, mean), put(s.rstd, rstd), put(s.y, _round(y, c.dtype))
        else:
            dy = _round(gemm(s.dy, True), c.dtype) if isinstance(s.dy, R.Gemm) else val(s.dy)
            x, mean, rstd, gamma = val(s.x), val(s.mean), val(s.rstd), val(s.gamma)
            n = F32(c.D)
            xh = (x - mean[:, None]) * rstd[:, None]
            g = dy * gamma
            s1 = g.sum(1, dtype=F32) / n
            s2 = (g * xh).sum(1, dtype=F32) / n
            dx = rstd[:, None] * (g - s1[:, None] - (F32(0) if wrong == "s2_dropped" else xh * s2[:, None]))
            k = R.keep_scale(c, c.D, s.p if s.mode else 0.0, s.site).astype(F32)
            if s.mode == 2:
                dx = dx * k if wrong == "mode2_k" else dx * (F32(1) + k)
            put(s.dx, _round(dx, c.dtype))
            if s.mode == 1:
                put(s.dxm, _round(dx * k, c.dtype))
            # the parameter gradients: one partial row per part, added in index order
            P = R.n_parts(c)
            edges = np.linspace(0, c.M, P + 1).astype(int) if c.kind == "ln" else np.minimum(np.arange(P + 1) * 64, c.M)
            if wrong == "dgamma_ragged_tile_lost":
                edges = np.minimum(edges, c.M // 64 * 64)
            tg, tb = dy * xh, dy
            parts = np.stack([np.concatenate([tg[a:b].sum(0, dtype=F32), tb[a:b].sum(0, dtype=F32)]) for a, b in zip(edges[:-1], edges[1:])])
            if wrong == "dgamma_row_twice":
                parts[-1] += np.concatenate([tg[-1], tb[-1]])
            if s.parts:
                outs[s.parts][:P] = torch.from_numpy(parts)
            tot = F32(R.INIT) + parts.sum(0, dtype=F32)
            put(s.dgamma, tot[:c.D]), put(s.dbeta, tot[c.D:])
    return outs


_CACHE = {}


def evaluated(c):
    """(operands, fp32 evaluation, stage results) of a case, computed once"""
    if c.id not in _CACHE:
        ins = R.operands(c)
        outs = emulate(c, ins)
        _CACHE[c.id] = (ins, outs, R.check(c, ins, outs))
    return _CACHE[c.id]


# ------------------------------------------------------------------------------------------ the reference is right
def _indep_rows(c):
    """the physical row of every logical row, written out as the header states it"""
    if c.groups is None:
        return list(range(c.M))
    rpg, stride, off = c.groups
    return [(m // rpg) * stride + off + (m % rpg) for m in range(c.M)]


def _tval(c, bufs, ins, outs, name):
    b = bufs[name]
    t = (outs[name] if b.out else ins[name]).double()
    if b.rows == "log":
        return t[:c.M, :b.width]
    if b.rows == "phys":
        return t[_indep_rows(c), :b.width]
    if b.rows == "stat":
        return t[_indep_rows(c)]
    if b.rows == "vec":
        return t[:b.width]
    return t[:, :b.width]


def _tkeep(c, N, p, site):
    if p <= 0:
        return torch.ones((c.M, N), dtype=torch.float64)
    pr = np.array(_indep_rows(c), dtype=np.uint64)
    idx = pr[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    keep, _ = R.keep_mask(R.SEED ^ R.SEED_WORD, site, idx, p)
    thr = int(np.float32(p) * np.float32(65536.0))
    return torch.from_numpy(keep.astype(np.float64)) * (65536.0 / (65536.0 - thr))


def _tgemm(c, bufs, ins, outs, s):
    v = lambda n: _tval(c, bufs, ins, outs, n)  # noqa: E731
    t = v(s.A) @ v(s.B).T
    if s.bias:
        t = t + v(s.bias)
    t = t * float(np.float32(s.alpha))
    if s.relu:
        t = torch.relu(t)
    if s.p > 0:
        u = t * _tkeep(c, t.shape[1], s.p, s.site)
    else:
        u = t
    t = t + u if s.self_resid else u
    if s.resid:
        t = t + v(s.resid)
    if s.gate:
        t = t * (v(s.gate) > 0)
    return t


@pytest.mark.parametrize("cid", IDS)
def test_the_reference_equals_torch_autograd_in_fp64(cid):
    """every stage's reference against torch.nn.functional.layer_norm, plain matmuls and autograd in fp64, on the case's operands and
    the stored tensors of its fp32 evaluation; the row maps, the three mask modes and the (1 + k) form are written out here again"""
    c = case(cid)
    ins, outs, results = evaluated(c)
    bufs, stages = R.plan(c)
    v = lambda n: _tval(c, bufs, ins, outs, n)  # noqa: E731
    want = {}
    for s in stages:
        if isinstance(s, R.Gemm):
            want[s.out] = _tgemm(c, bufs, ins, outs, s)
        elif isinstance(s, R.LnFwd):
            h = v(s.h)
            want[s.y] = torch.nn.functional.layer_norm(h, (c.D,), v(s.gamma), v(s.beta), eps=R.EPS)
            want[s.mean] = h.mean(1)
            want[s.rstd] = (h.var(1, unbiased=False) + R.EPS).rsqrt()
        else:
            dy = _tgemm(c, bufs, ins, outs, s.dy) if isinstance(s.dy, R.Gemm) else v(s.dy)
            x, gamma, mean, rstd = v(s.x), v(s.gamma), v(s.mean), v(s.rstd)
            k = _tkeep(c, c.D, s.p if s.mode else 0.0, s.site)
            # (1) with the exact statistics of x the reference's functions equal autograd straight through layer_norm
            xg, gg, bg = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), torch.zeros(c.D, dtype=torch.float64, requires_grad=True)
            y = torch.nn.functional.layer_norm(xg, (c.D,), gg, bg, eps=R.EPS)
            ax, ag, ab = torch.autograd.grad(y, (xg, gg, bg), dy)
            mu = x.mean(1)
            r = R.ln_bwd_ref(dy.numpy(), x.numpy(), mu.numpy(), (x.var(1, unbiased=False) + R.EPS).rsqrt().numpy(), gamma.numpy(), k.numpy(),
                             s.mode, c.dtype)
            auto = {"dx": ax + ax * k if s.mode == 2 else ax, "dxm": ax * k, "dgamma": R.INIT + ag, "dbeta": R.INIT + ab}
            for key, (ref, _) in r.items():
                w = auto[key].numpy()
                assert np.abs(ref - w).max() <= 1e-12 * max(1.0, float(np.abs(w).max())), f"{c.id}: {key} against autograd"
            # (2) with the statistics the launch is handed (fp32: not exactly those of x) the same formulas, written out here
            xh = (x - mean[:, None]) * rstd[:, None]
            g = dy * gamma
            dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
            if s.mode == 2:
                want[s.dx] = dx + dx * k
            else:
                want[s.dx] = dx
                if s.mode == 1:
                    want[s.dxm] = dx * k
            want[s.dgamma], want[s.dbeta] = R.INIT + (dy * xh).sum(0), R.INIT + dy.sum(0)
    assert len(results) == len(want)
    for r in results:
        w = want[r.name].detach().numpy()
        scale = max(1.0, float(np.abs(w).max()))
        assert np.abs(r.ref - w).max() <= 1e-12 * scale, f"{c.id}: {r.name} ({r.stage})"


# ------------------------------------------------------------------------------------------ the bound takes what it must
@pytest.mark.parametrize("cid", IDS)
def test_the_bounds_take_an_fp32_evaluation_in_another_order(cid):
    c = case(cid)
    ins, outs, results = evaluated(c)
    for r in results:
        assert not r.bad.any(), R.describe(c, r)
        # a bound of the size of the result would accept anything
        if r.ref.ndim == 2:
            assert np.median(r.bound) < 0.05 * np.abs(r.ref).max(), f"{c.id}: {r.name}"
    assert R.intact(c, outs) == []
    print(f"\n{c.id}: worst fp32 error / bound " + ", ".join(f"{r.name} {r.ratio:.3f}" for r in results))


# ------------------------------------------------------------------------------------------ the bound refuses what it must
def _share(c, wrong, name, affected):
    """the share of the affected elements of tensor `name` that land outside the bound when the launch makes mistake `wrong`"""
    ins = R.operands(c)
    outs = emulate(c, ins, wrong)
    r = [x for x in R.check(c, ins, outs) if x.name == name]
    assert len(r) == 1
    bad = r[0].bad
    sel = affected(r[0]) if callable(affected) else affected
    assert sel.any()
    share = float(bad[sel].mean())
    print(f"{c.id}: {wrong}: {name}: {share:.3f} of {int(sel.sum())} affected elements outside the bound")
    return share


def _rows_mask(c, rows_):
    m = np.zeros(c.M, dtype=bool)
    m[rows_] = True
    return m


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_the_bounds_refuse_wrong_statistics(dtype):
    dn = R.DT_NAME[dtype]
    c = case(f"ln-{dn}-M1000-D128-g1_1_0-m2")       # x is an input: its offset and constant rows are where operands() put them
    offset = np.arange(c.M) % 8 == R.OFFSET_ROW
    const = _rows_mask(c, [R.CONST_ROW])
    # E[x^2] - mean^2 in fp32 on rows with mean^2 / var = 64 / 0.008: one rounding at 64 is 2^-24 * 64 = 4e-6 against a bound of
    # var (n + 21) 2^-24 = 7e-8 (n = 128) or 5e-7 (n = 1024). The rows' values are sixteenths (exact in both types), so the sum of
    # their squares often still fits fp32's 24 bits and only mean * mean rounds, and not where the mean has few bits: most rows, not all
    assert _share(c, "one_pass_var", "rstd", offset) >= 0.5
    assert _share(case(f"ln-{dn}-M1000-D1024-g1_1_0-m1"), "one_pass_var", "rstd", offset) >= 0.5
    # eps decides rstd alone on the constant row and moves it by 6e-4 on the offset rows; the bound there is 5e-6
    for w in ("eps_1e-6", "eps_outside_root"):
        assert _share(c, w, "rstd", offset | const) == 1.0, w
    # n / (n - 1) under the root: 1 / (2 n) = 4e-3 in every row that has a variance
    assert _share(c, "unbiased_var", "rstd", ~const) >= 0.99
    c = case(f"ln-{dn}-M1000-D1024-g1_1_0-m1")
    assert _share(c, "unbiased_var", "rstd", ~_rows_mask(c, [R.CONST_ROW])) >= 0.99  # 5e-4 against (n + 21) 2^-25 = 3e-5
    # statistics of the row BEFORE its 16-bit rounding: n rounding errors, uniform within u_out |h|, move the mean by a normal
    # deviate of sigma = u_out |h| / sqrt(3 n); the fp32 bound is (n + 16) 2^-24 |h|. The share of rows outside it is therefore
    # erfc(bound / (sigma sqrt 2)): all but a few in bf16, and in fp16 0.73 at n = 128, 0.36 at n = 256, where eleven bits of
    # rounding in 256 elements are no more than fp32's own error bound
    for cid, n in ((f"ffn_fwd-{dn}-M1637-D128-F512-self", 128), (f"gemm_ln_fwd-{dn}-M200-D256-F1024-g50_53_2", 256)):
        c = case(cid)
        sigma, bound = R.u_out(dtype) / math.sqrt(3 * n), (n + 16) * R.U
        expect = math.erfc(bound / (sigma * math.sqrt(2)))
        assert _share(c, "unrounded_stats", "mean", np.ones(c.M, dtype=bool)) >= expect - 0.1, (cid, expect)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_the_bounds_refuse_a_wrong_backward(dtype):
    dn = R.DT_NAME[dtype]
    # xh mean(g xh) left out: of the size |xh| |g| / sqrt(n) against u_out |dx|; nothing to see where xh is small or on the constant row
    c = case(f"ln-{dn}-M1000-D128-g1_1_0-m2")
    assert _share(c, "s2_dropped", "dx", lambda r: np.abs(r.ref) > 0) >= 0.8
    c = case(f"gemm_ln_bwd-{dn}-M200-D128-F128-g64_65_1-m2")
    assert _share(c, "s2_dropped", "dx", lambda r: np.abs(r.ref) > 0) >= (0.5 if dtype == R.BF else 0.8)
    # dx k where mode 2 wants dx (1 + k): off by dx itself
    for cid in (f"ln-{dn}-M1000-D128-g1_1_0-m2", f"gemm_ln_bwd-{dn}-M200-D128-F128-g64_65_1-m2", f"gemm_ln_bwd-{dn}-M200-D256-F128-m2-p0"):
        c = case(cid)
        assert _share(c, "mode2_k", "dx", lambda r: np.abs(r.ref) > 0) >= 0.95, cid
    # the mode-2 residual taken at the physical row under (50, 53, 2): every row's residual is another row's
    c = case(f"gemm_ln_bwd-{dn}-M1637-D128-F1024-g50_53_2-m2")
    assert _share(c, "resid_phys", "dx", lambda r: np.abs(r.ref) > 0) >= 0.9
    # the rows of the ragged last tile (37 of 1637) missing from dgamma / dbeta, and one row counted twice: on a stage whose dy is a
    # stored tensor (the leading LayerNorm backward) the bound is 2 (M + 16) 2^-24 = 2e-4 of the sum of magnitudes, a third of the
    # AVERAGE term: 37 terms show in every column, a single one (the mistake here: one row counted twice) where it is not among the column's small ones
    for cid in (f"ffn_bwd-{dn}-M1637-D128-F512-lead0", f"ffn_bwd-{dn}-M1637-D256-F1024-lead1"):
        c = case(cid)
        for name in ("l_dgamma", "l_dbeta"):
            assert _share(c, "dgamma_ragged_tile_lost", name, np.ones(c.D, dtype=bool)) >= 0.95, (cid, name)
            assert _share(c, "dgamma_row_twice", name, np.ones(c.D, dtype=bool)) >= 0.5, (cid, name)
    # ... and behind a GEMM whose result is not stored, dy carries the GEMM's whole bound e, and sum(e |xh|) adds u_out |dy| over
    # 1637 rows without cancellation. In fp16 a whole lost tile still shows in dbeta's columns. In bf16 that worst-case term is about
    # as large as 37 missing rows, so a lost tile in the MAIN dgamma / dbeta of mst_ffn_ln_bwd or mst_gemm_nt_ln mode 2 could pass
    # the bound: a known gap of a correct worst-case bound. What covers a lost tile there: the partial rows (one per tile, NaN
    # before the launch, checked for NaN after it) and the leading-LayerNorm cases above, whose dy is stored
    c = case(f"gemm_ln_bwd-{R.DT_NAME[R.FP]}-M1637-D128-F128-m0")
    assert _share(c, "dgamma_ragged_tile_lost", "dbeta", np.ones(c.D, dtype=bool)) >= 0.5


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_the_bounds_refuse_the_dropout_counter_at_the_logical_row(dtype):
    dn = R.DT_NAME[dtype]
    for cid, name, N, site in ((f"ffn_fwd-{dn}-M1664-D128-F512-g64_65_1-rg", "a", 512, R.SITE_FF1),
                               (f"ffn_fwd-{dn}-M1664-D128-F512-g64_65_1-proj-rg", "h1", 128, R.SITE_PROJ)):
        c = case(cid)
        differ = R.keep_scale(c, N, c.p, site) != R.keep_scale(c, N, c.p, site, np.arange(c.M))
        assert 0.25 < differ.mean() < 0.4  # 2 p (1 - p) = 0.32
        # (the hidden activation is zero on either side where the ReLU closed it)
        sel = (lambda r: differ & (np.abs(r.ref) + np.abs(r.got) > 0)) if name == "a" else differ
        assert _share(c, "logical_counter", name, sel) >= 0.95, cid


# ------------------------------------------------------------------------------------------ the cases reach what they are meant for
def test_the_table_reaches_every_ffn_ln_kernel_and_every_chunk_rotation():
    for dtype in R.DTYPES:
        for D in (128, 256):
            cs = [c for c in R.CASES if c.dtype == dtype and c.D == D and c.kind in ("ffn_fwd", "ffn_bwd")]
            assert {R.ffn_kernel_index(c) for c in cs} == set(range(8)), (dtype, D)
            for c in cs:
                assert c.F % c.D == 0
                tiles = (c.M + 63) // 64
                if c.F // c.D == 4:
                    assert tiles >= 25 and {(w // 8) % 4 for w in range(tiles)} == {0, 1, 2, 3}, c.id
                if c.groups is not None:
                    assert c.M % c.groups[0] == 0 and c.groups[0] % 64 == 0
            assert {c.F // c.D for c in cs} == ({1, 4} if D == 128 else {2, 4})
            assert any(c.M % 64 and ((c.M + 63) // 64) % 8 for c in cs), "a ragged last tile in a grid that is no multiple of 8"
        fwd = [c for c in R.CASES if c.dtype == dtype and c.kind == "ffn_fwd"]
        assert {c.resid for c in fwd} == {"x", "self", "other"} and any(c.p == 0 for c in fwd) and any(c.groups for c in fwd)
        assert any(c.proj and c.groups for c in fwd)
        bwd = [c for c in R.CASES if c.dtype == dtype and c.kind == "ffn_bwd"]
        assert {c.mode for c in bwd if c.lead < 0} == {0, 1, 2} and {c.lead for c in bwd} == {-1, 0, 1}
        assert {c.partials for c in bwd} == {True, False} and any(c.alpha != 1 for c in bwd) and any(c.groups for c in bwd)
        assert {(c.D, c.M % 64 == 0) for c in bwd if c.lead >= 0} == {(128, True), (128, False), (256, True), (256, False)}
        for kind in ("gemm_ln_fwd", "gemm_ln_bwd"):
            g = [c for c in R.CASES if c.dtype == dtype and c.kind == kind]
            assert {c.D for c in g} == {128, 256} and {c.F for c in g} == {128, 1024} and {c.M for c in g} == {64, 200, 1637}
            assert {c.groups for c in g} == {None, (64, 65, 1), (50, 53, 2)}
        g = [c for c in R.CASES if c.dtype == dtype and c.kind == "gemm_ln_bwd"]
        assert {c.mode for c in g} == {0, 1, 2} and {c.partials for c in g} == {True, False}
        ln = [c for c in R.CASES if c.dtype == dtype and c.kind == "ln"]
        assert {c.D for c in ln} == {32, 40, 128, 256, 260, 512, 772, 1024}
        assert {c.M for c in ln} == {16, 77, 1000, 1025, 1029, 8192, 8193, 8197, 16389}
        assert {c.groups[1] for c in ln} == {1, 4} and {c.mode for c in ln} == {0, 1, 2} and {c.partials for c in ln} == {True, False}
        assert sum(c.kind == "dec_tail" and c.dtype == dtype for c in R.CASES) == 1
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("cid", IDS)
def test_the_operands_are_hard(cid):
    c = case(cid)
    bufs, _ = R.plan(c)
    ins = R.operands(c)
    outs = R.outputs(c)
    hard = [n for n, b in bufs.items() if not b.out and b.rows in ("log", "phys") and n not in ("gate", "dy", "dyl", "dff")]
    assert hard
    for n in hard:
        x = R.gather(c, bufs[n], ins[n])
        shift = R.LEAD_SHIFT if n == "xl" else 0
        assert np.ptp(x[R.CONST_ROW + shift]) == 0 and x[R.CONST_ROW + shift, 0] != 0, f"{n}: a constant row"
        o = x[R.OFFSET_ROW]
        assert abs(o.mean()) > 20 * o.std() > 0, f"{n}: a row whose offset is much larger than its spread"
        s = x[R.SPIKE_ROW + shift]
        assert np.abs(s).max() > 30 * np.median(np.abs(s)), f"{n}: a row with one large element"
    for n, b in bufs.items():
        if b.rows == "vec" and n in ("gamma", "g1", "gl"):
            g = ins[n].numpy()
            assert g[R.ZERO_GAMMA] == 0 and (g < 0).any() and (g > 0).any() and np.abs(g).max() > 2 and np.abs(g[g != 0]).min() < 0.5
        if b.rows == "vec" and n in ("beta", "be1"):
            assert (ins[n] != 0).all()
        if b.out:
            t = outs[n]
            if b.rows == "parts":
                assert t.isnan().all() and t.shape[0] == b.n + 1
            else:
                own = R.owned(c, b)
                assert (t.float().numpy()[~own] == R.SENTINEL).all()
                if b.rows in ("log", "phys"):
                    assert t.shape[1] == b.width + 8 and (~own[-R.GUARD:]).all() and (~own[:, b.width:]).all()
        elif b.rows in ("log", "phys", "w"):
            t = ins[n].float().numpy()
            own = R.owned(c, b)
            assert np.isnan(t[~own]).all() and np.isfinite(t[own]).all() and t.shape[1] == b.width + 8
            # (rows of 16 bytes for the GEMM launches; the stand-alone LayerNorm loads 8 bytes and takes any multiple of 4: D = 260)
            assert ins[n].stride(0) % (4 if c.kind == "ln" else 8) == 0
            if c.groups is not None and b.rows == "phys" and c.kind != "ln":
                assert (~own).any(1).all() and (~own).all(1).any(), f"{n}: rows outside the groups hold NaN"
        elif b.rows == "stat":
            t = ins[n].numpy()
            own = R.owned(c, b)
            assert np.isnan(t[~own]).all() and np.isfinite(t[own]).all()


# ------------------------------------------------------------------------------------------ the stand-alone kernels, form by form
LN = [c for c in R.CASES if c.kind == "ln"]
LN_NEW = [c for c in LN if (c.M, c.D) in R.LN_FORMS]


@pytest.fixture(scope="module")
def ops():
    from musicstyletransfer_amd import ops as o
    o._lib.load()
    return o


def test_the_ln_cases_reach_every_instantiation_the_dispatcher_has(ops):
    """asked of the library (mst_layernorm_form: no HIP call): each case runs the <NV, R> it claims, the restated ln_form agrees with
    the query field by field, and between them the cases leave no (NV, R) pair of either direction unclaimed"""
    for dtype in R.DTYPES:
        fwd, bwd = set(), set()
        for c in (c for c in LN if c.dtype == dtype):
            f, b = ops.layernorm_form(False, c.dtype, c.M, c.D), ops.layernorm_form(True, c.dtype, c.M, c.D)
            assert (f["nv"], f["r"], b["r"]) == c.form and b["nv"] == f["nv"], (c.id, f, b)
            for back, q in ((False, f), (True, b)):
                assert R.ln_form(back, c.M, c.D) == (q["nv"], q["r"], q["grid"], q["waves"], q["lds"]), c.id
            assert b["grid"] == R.n_parts(c) == ops.layernorm_bwd_parts(c.M, c.D)
            fwd.add((f["nv"], f["r"])), bwd.add((b["nv"], b["r"]))
        # what the dispatcher can produce at all: every (NV, R) the query returns over a sweep of shapes around every threshold
        can_f, can_b = set(), set()
        for D in (4, 32, 256, 260, 512, 516, 1024):
            for M in (1, 16, 1024, 1025, 4096, 8192, 8193, 16384, 16385, 70000):
                f, b = ops.layernorm_form(False, dtype, M, D), ops.layernorm_form(True, dtype, M, D)
                can_f.add((f["nv"], f["r"])), can_b.add((b["nv"], b["r"]))
        assert can_f == {(nv, r) for nv in (1, 2, 4) for r in (1, 2)} and can_b == {(1, 1), (1, 2), (2, 1), (4, 1)}
        assert fwd == can_f and bwd == can_b
        new = [c for c in LN_NEW if c.dtype == dtype]
        # the boundary, the 256-workgroup cap with an odd number of trips, a partly empty last lane group at NV = 2 and 4
        assert {ops.layernorm_form(False, dtype, M, 32)["r"] for M in (8192,)} == {1} and R.ln_form(False, 8193, 32)[1] == 2
        assert any(R.ln_form(True, c.M, c.D)[2] == 256 and -(-c.M // (256 * 16 * 2)) % 2 == 1 and not c.partials for c in new)
        assert any(R.ln_form(True, c.M, c.D)[2] == 256 and c.partials for c in new)
        assert {nv for c in new for nv in [R.ln_form(False, c.M, c.D)[0]] if (c.D // 4) % 64} >= {1, 2, 4}
        assert any(c.groups[1] > 1 and c.mode == m and c.p > 0 and c.form[2] == 2 for c in new for m in (1,)) \
            and any(c.groups[1] > 1 and c.mode == 2 and c.p > 0 and c.form[2] == 2 for c in new)
    with pytest.raises(ops._lib.MstError, match="multiple of 4"):
        ops.layernorm_form(False, torch.bfloat16, 8, 6)
    with pytest.raises(ops._lib.MstError, match="must be positive"):
        ops.layernorm_form(True, torch.bfloat16, 0, 8)
    with pytest.raises(ops._lib.MstError, match="<= 1024"):
        ops.layernorm_form(True, torch.float16, 8, 1028)


def _tree64(x):
    """the sum over the 64 lanes (last axis) as a butterfly: 32 + 32, 16 + 16, ..."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _lanes(t, nv):
    """[M, D] -> [M, NV, 64, 4]: element 4 (64 i + lane) + e at [i, lane, e], zeros behind D as the kernel's registers hold them"""
    M, D = t.shape
    out = torch.zeros((M, nv * 256), dtype=torch.float32)
    out[:, :D] = t
    return out.view(M, nv, 64, 4)


def emulate_ln(c, ins, wrong=None):
    """the two stand-alone launches of an "ln" case in torch fp32, in the kernels' order: a row's elements dealt to 64 lanes in NV groups
    of 4, per-lane sums in the kernel's association, a butterfly over the lanes, two-pass variance over the live lane groups only; rows
    dealt to waves as `for m0 = wave; m0 < M; m0 += nwaves * R` with rows m0 and m0 + nwaves in flight; the parameter gradients summed
    per wave in row order, over the waves of a workgroup in index order, then per workgroup (a partial row each, or added to the
    initial value in index order). wrong: one mistake a kernel of this shape can make (the list is the issue's). -> the output buffers"""
    f32 = torch.float32
    bufs, _ = R.plan(c)
    outs = R.outputs(c)
    M, D, stride = c.M, c.D, c.groups[1]
    T = lambda name: torch.from_numpy(R.gather(c, bufs[name], ins[name])).to(f32)  # noqa: E731
    x, dy, gamma, beta = T("x"), T("dy"), T("gamma"), T("beta")
    n_live = D // 4
    sentinel = torch.tensor(R.SENTINEL, dtype=f32)

    def pairs(back):
        """-> (second-row flag of every row, index of its pair partner or -1)"""
        nv, r, grid, nw, _ = R.ln_form(back, M, D)
        nwaves = grid * nw
        m = np.arange(M)
        if r == 1:
            return nv, nwaves, np.zeros(M, dtype=bool), np.full(M, -1)
        second = (m // nwaves) % 2 == 1
        partner = np.where(second, m - nwaves, m + nwaves)
        return nv, nwaves, second, np.where(partner < M, partner, -1)

    # ---------------- forward
    nv, nwaves, second, partner = pairs(False)
    v = _lanes(x, nv)
    s = torch.zeros((M, 64), dtype=f32)
    for i in range(nv):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    inv_d = torch.tensor(1.0, dtype=f32) / torch.tensor(float(D), dtype=f32)
    mean = _tree64(s) * inv_d
    live = (torch.arange(nv * 64).view(nv, 64) < n_live)  # [NV, 64]
    ss = torch.zeros((M, 64), dtype=f32)
    for i in range(nv):
        for e in range(4):
            d = v[:, i, :, e] - mean[:, None]
            sq = d * d
            ss = ss + (sq if wrong == "empty_group_counted" else torch.where(live[i][None, :], sq, torch.zeros((), dtype=f32)))
    var = _tree64(ss) * (torch.tensor(1.0, dtype=f32) / torch.tensor(float(D - 1), dtype=f32) if wrong == "unbiased_var" else inv_d)
    eps = torch.tensor(1e-5, dtype=f32)
    rstd = 1.0 / (torch.sqrt(var) + eps) if wrong == "eps_outside_root" else 1.0 / torch.sqrt(var + eps)
    if wrong == "pair_stats_swapped":
        both = torch.from_numpy(partner >= 0)
        idx = torch.from_numpy(np.where(partner >= 0, partner, np.arange(M)))
        mean, rstd = torch.where(both, mean[idx], mean), torch.where(both, rstd[idx], rstd)
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    done = np.ones(M, dtype=bool)
    if wrong == "pair_second_dropped":   # the second row's liveness tested as m + 1 < M
        done = ~(second & (np.arange(M) == M - 1))
    dn = torch.from_numpy(done)
    R.scatter(c, bufs["y"], outs["y"], torch.where(dn[:, None], y.to(c.dtype).float(), sentinel).numpy())
    if wrong == "stats_at_m":            # statistics stored at m, not m * row_id_stride
        outs["mean"][:M], outs["rstd"][:M] = mean, rstd
    else:
        R.scatter(c, bufs["mean"], outs["mean"], torch.where(dn, mean, sentinel).numpy())
        R.scatter(c, bufs["rstd"], outs["rstd"], torch.where(dn, rstd, sentinel).numpy())
    # ---------------- backward, on the statistics the forward stored
    mean = torch.from_numpy(R.gather(c, bufs["mean"], outs["mean"])).to(f32)
    rstd = torch.from_numpy(R.gather(c, bufs["rstd"], outs["rstd"])).to(f32)
    nv, nwaves, second, partner = pairs(True)
    _, _, grid, nw, _ = R.ln_form(True, M, D)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    gl, gxl = _lanes(g, nv), _lanes(g * xh, nv)
    s1, s2 = torch.zeros((M, 64), dtype=f32), torch.zeros((M, 64), dtype=f32)
    for i in range(nv):
        for e in range(4):
            s1, s2 = s1 + gl[:, i, :, e], s2 + gxl[:, i, :, e]
    s1, s2 = _tree64(s1) * inv_d, _tree64(s2) * inv_d
    dx = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
    p = c.p if c.mode else 0.0
    if p > 0:
        counter = np.arange(M) if wrong == "counter_from_m" else R.rows(c)[0]
        idx = counter.astype(np.uint64)[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :]
        keep, scale = R.keep_mask(R.SEED if wrong == "seed_ignored" else R.SEED ^ R.SEED_WORD, R.SITE_LN, idx, p)
        k = torch.from_numpy(keep * scale).to(f32)
    else:
        k = torch.ones((M, D), dtype=f32)
    done = np.ones(M, dtype=bool)
    if wrong == "pair_second_dropped":
        done = ~(second & (np.arange(M) == M - 1))
    dn = torch.from_numpy(done)[:, None]
    main = dx * (1.0 + k) if c.mode == 2 else dx
    R.scatter(c, bufs["dx"], outs["dx"], torch.where(dn, main.to(c.dtype).float(), sentinel).numpy())
    if c.mode == 1:
        R.scatter(c, bufs["dxm"], outs["dxm"], torch.where(dn, (dx * k).to(c.dtype).float(), sentinel).numpy())
    acc = torch.zeros((nwaves, 2 * D), dtype=f32)
    terms = torch.cat([dy * xh, dy], 1) * torch.from_numpy(done)[:, None]
    for j in range(-(-M // nwaves)):
        rows_ = terms[j * nwaves:(j + 1) * nwaves]
        acc[:rows_.shape[0]] += rows_
    wg = torch.zeros((grid, 2 * D), dtype=f32)
    for w in range(nw):
        wg += acc.view(grid, nw, 2 * D)[:, w]
    tot = torch.full((2 * D,), R.INIT, dtype=f32)
    for b in range(grid):
        tot = tot + wg[b]
    if c.partials:
        outs["parts"][:grid] = wg
    R.scatter(c, bufs["dgamma"], outs["dgamma"], tot[:D].numpy()), R.scatter(c, bufs["dbeta"], outs["dbeta"], tot[D:].numpy())
    return outs


_LN_CACHE = {}


def _ln_eval(c):
    if c.id not in _LN_CACHE:
        ins = R.operands(c)
        _LN_CACHE[c.id] = (ins, emulate_ln(c, ins))
    return _LN_CACHE[c.id]


@pytest.mark.parametrize("c", LN_NEW, ids=lambda c: c.id)
def test_the_bounds_take_the_kernels_own_order(c):
    ins, outs = _ln_eval(c)
    results = R.check(c, ins, outs)
    print(f"\n{c.id}: worst fp32 (kernel order) error / bound " + ", ".join(f"{r.name} {r.ratio:.3f}" for r in results))
    for r in results:
        assert not r.bad.any(), R.describe(c, r)
    assert R.intact(c, outs) == []


def _ln_share(c, wrong, name, sel):
    ins, _ = _ln_eval(c)
    r = [x for x in R.check(c, ins, emulate_ln(c, ins, wrong)) if x.name == name]
    assert len(r) == 1
    sel = sel(r[0]) if callable(sel) else sel
    assert sel.any(), (c.id, wrong, name)
    share = float(r[0].bad[sel].mean())
    print(f"{c.id}: {wrong}: {name}: {share:.3f} of {int(sel.sum())} affected elements outside the bound")
    return share


@pytest.mark.parametrize("c", LN_NEW, ids=lambda c: c.id)
def test_the_bounds_refuse_what_a_wrong_pair_kernel_stores(c):
    """every mistake in every case suited to it (a case is suited where the mistake changes what is stored)"""
    M, D, stride = c.M, c.D, c.groups[1]
    m = np.arange(M)
    const = _rows_mask(c, [R.CONST_ROW])
    tried = set()
    for back, names in ((False, ("y", "mean", "rstd")), (True, ("dx",))):
        nv, r, grid, nw, _ = R.ln_form(back, M, D)
        nwaves = grid * nw
        if r == 2:
            second = (m // nwaves) % 2 == 1
            if second[M - 1]:   # the row is never stored: the sentinel stays, in every element
                for name in names:
                    sel = (m == M - 1) if name in ("mean", "rstd") else np.broadcast_to((m == M - 1)[:, None], (M, D))
                    # (an element of y or dx may itself lie at the sentinel, 7: gamma reaches 4)
                    assert _ln_share(c, "pair_second_dropped", name, sel) >= (1.0 if name in ("mean", "rstd") else 0.95)
                tried.add("pair_second_dropped")
            if not back:
                partner = np.where(second, m - nwaves, m + nwaves)
                both = partner < M
                # two rows' means differ by far more than (n + 16) u mean|h| unless both are offset rows (8 + sixteenths: their means
                # are 0.1 apart at most) or chance has it
                assert _ln_share(c, "pair_stats_swapped", "mean", both) >= 0.95
                tried.add("pair_stats_swapped")
    if stride > 1:
        # index m holds row m's statistics, index m * stride is read: another row's (or the sentinel)
        assert _ln_share(c, "stats_at_m", "mean", m > 0) >= 0.95
        tried.add("stats_at_m")
        if c.mode and c.p > 0:
            name = "dxm" if c.mode == 1 else "dx"
            differ = R.keep_scale(c, D, c.p, R.SITE_LN) != R.keep_scale(c, D, c.p, R.SITE_LN, m)
            assert 0.25 < differ[1:].mean() < 0.4   # 2 p (1 - p) = 0.32 (row 0: the same counter either way)
            # a decision the other way moves the element by its own size (mode 1: dx / 0.8 against 0; mode 2: dx against 2.25 dx)
            assert _ln_share(c, "counter_from_m", name, lambda r: differ & (np.abs(r.ref) + np.abs(r.got) > 0)) >= 0.95
            tried.add("counter_from_m")
    if c.mode and c.p > 0:
        name = "dxm" if c.mode == 1 else "dx"
        idx = R.rows(c)[0].astype(np.uint64)[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :]
        differ = R.keep_mask(R.SEED, R.SITE_LN, idx, c.p)[0] != R.keep_mask(R.SEED ^ R.SEED_WORD, R.SITE_LN, idx, c.p)[0]
        assert 0.25 < differ.mean() < 0.4
        assert _ln_share(c, "seed_ignored", name, lambda r: differ & (np.abs(r.ref) + np.abs(r.got) > 0)) >= 0.95
        tried.add("seed_ignored")
    if (D // 4) % 64:
        # e = 256 NV - D zeros, each counted as mean^2: the variance grows by mean^2 e / D. A unit-scale row has mean = z / sqrt(D) with z
        # a standard normal deviate, so rstd moves by z^2 e / (2 D^2) of itself against a bound of about (D + 20) u / 2: refused where
        # z^2 > (D + 20) u D^2 / e, a share of erfc(sqrt(that / 2)) of the rows (0.95 at D = 260, 0.74 at D = 772); the constant row
        # (variance 0, mean 3) and the offset rows (mean 8) by orders of magnitude
        e = 256 * R.ln_form(False, M, D)[0] - D
        expect = math.erfc(math.sqrt((D + 20) * R.U * D * D / e / 2))
        assert _ln_share(c, "empty_group_counted", "rstd", np.ones(M, dtype=bool)) >= expect - 0.05, expect
        assert _ln_share(c, "empty_group_counted", "rstd", const | (m % 8 == R.OFFSET_ROW)) == 1.0
        tried.add("empty_group_counted")
    # n / (n - 1) under the root: 1 / (2 n) of rstd in every row that has a variance, against (n + 20) u / 2
    assert _ln_share(c, "unbiased_var", "rstd", ~const) >= 0.99
    # eps decides rstd alone on the constant row; on the offset rows (var about 0.008) it moves it by 6e-4 against a bound of 5e-6
    assert _ln_share(c, "eps_outside_root", "rstd", const | (m % 8 == R.OFFSET_ROW)) == 1.0
    want = {"unbiased_var", "eps_outside_root"} | tried
    print(f"{c.id}: refused {sorted(want)}")


def test_every_pair_mistake_has_a_case():
    """the mistakes that need a shape of their own are each refused in at least one case per type (which: the test above prints)"""
    for dtype in R.DTYPES:
        new = [c for c in LN_NEW if c.dtype == dtype]
        f = lambda c, back: R.ln_form(back, c.M, c.D)  # noqa: E731
        def second_last(c, back):
            nv, r, grid, nw, _ = f(c, back)
            return r == 2 and ((c.M - 1) // (grid * nw)) % 2 == 1
        assert any(second_last(c, False) for c in new) and any(second_last(c, True) for c in new)
        assert any(c.groups[1] > 1 and f(c, True)[1] == 2 and c.mode == 1 for c in new)
        assert any(c.groups[1] > 1 and f(c, True)[1] == 2 and c.mode == 2 for c in new)
        assert {f(c, False)[0] for c in new if (c.D // 4) % 64 and f(c, False)[1] == 2} == {1, 2, 4}
