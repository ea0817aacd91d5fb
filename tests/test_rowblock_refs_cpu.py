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
        assert {c.D for c in ln} == {32, 40, 128, 256, 1024} and {c.M for c in ln} == {16, 77, 1000}
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
            assert np.isnan(t[~own]).all() and np.isfinite(t[own]).all() and t.shape[1] == b.width + 8 and ins[n].stride(0) % 8 == 0
            if c.groups is not None and b.rows == "phys" and c.kind != "ln":
                assert (~own).any(1).all() and (~own).all(1).any(), f"{n}: rows outside the groups hold NaN"
        elif b.rows == "stat":
            t = ins[n].numpy()
            own = R.owned(c, b)
            assert np.isnan(t[~own]).all() and np.isfinite(t[own]).all()
