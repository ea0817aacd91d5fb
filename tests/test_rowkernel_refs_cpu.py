"""The references of tests/rowkernel_refs.py, checked without a GPU: each equals torch autograd or an answer worked by hand, the case
tables reach what they are meant for (the thread maps asked of the library's form query), every bound takes an fp32 evaluation of its
kernel (worst error / bound <= 1) and refuses each of a list of wrong kernels, and every refusal of the entry points comes with its
status and message before anything could be launched."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowkernel_refs as K  # noqa: E402

F32 = np.float32
EMBED_FWD = [c for c in K.EMBED_CASES if c.fwd]


@pytest.fixture(scope="module")
def ops():
    from musicstyletransfer_amd import ops as o
    o._lib.load()
    return o


def _to16(x32, dtype):
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).to(dtype)


# ------------------------------------------------------------------------------------------ fp32 evaluations, right and wrong
def emu_embed_fwd(c, ins, wrong=None, fused=False):
    out = K.embed_fwd_outputs(c)
    D = c.D
    tok = ins["tokens"].numpy().reshape(-1)
    r = np.arange(c.B * c.T)
    b, t = r // c.T, r % c.T
    kept = K._kept(c, ins)
    table = ins["table"].numpy()[:, :D]
    e = np.where(kept[:, None], table[np.where(kept, tok, 0)], F32(0))
    cc = np.zeros_like(e)
    if c.cls:
        cls_of = ins["classes"].numpy()[(r % c.B) if wrong == "class_of_row" else b]
        cc = ins["cls_table"].numpy()[cls_of, :D]
    prow = t if wrong == "pos_row_t" else c.s_off + t
    with np.errstate(invalid="ignore"):
        p = ins["pos"].numpy()[prow, :D]
        a = F32(c.alpha)
        s = (e + cc).astype(F32)
        v = (np.float64(a) * s.astype(np.float64) + p.astype(np.float64)).astype(F32) if fused else ((a * s).astype(F32) + p).astype(F32)
    rows_ = torch.from_numpy(K.embed_rows(c))
    out["out"][rows_, :D] = _to16(v, c.dtype)
    if c.keymask:
        km = (kept if wrong == "keymask_from_keep" else tok != 0).astype(np.uint8)
        out["keymask"][rows_] = torch.from_numpy(km)
    return out


def emu_colsum(X, idx, dst, T, D, s_off, S_out, alpha, wrong=None, skip=None):
    """group_colsum_kernel's thread map in fp32: chunks of 64 frames, a thread per 8 columns of every RG-th frame, the RG partial
    sums added in index order, one product, one addition into dst. X: fp32 [rows, >= D] flat; skip: frames left out ([B, T] bool)"""
    RG = 256 // (D // 8)
    a = F32(alpha)
    last = X.shape[0] - 1
    for b in range(len(idx)):
        for t0 in range(0, T, 64):
            t1 = t0 + 64 if wrong == "chunk_not_clipped" else min(t0 + 64, T)
            part = np.zeros((RG, D), dtype=F32)
            for t in range(t0, t1):
                if skip is not None and t < T and skip[b, t]:
                    continue
                row = b * S_out + (0 if wrong == "s_off_ignored" else s_off) + t
                part[(t - t0) % RG] += X[min(row, last), :D]
            v = np.zeros(D, dtype=F32)
            for g in range(RG):
                v = v + part[g]
            with np.errstate(invalid="ignore"):
                dst[idx[b], :D] += a * v


def emu_embed_bwd(c, ins, wrong=None, reverse=False):
    out = K.embed_bwd_outputs(c)
    D = c.D
    tok = ins["tokens"].numpy().reshape(-1)
    kept = K._kept(c, ins)
    use = np.ones_like(kept) if wrong == "dropped_scattered" else kept
    dX = ins["dX"].float().numpy()
    rows_ = K.embed_rows(c)
    order = np.nonzero(use)[0][::-1] if reverse else np.nonzero(use)[0]
    dt = out["dtable"].numpy()
    terms = (F32(c.alpha) * dX[rows_[order], :D]).astype(F32)
    np.add.at(dt, (tok[order][:, None], np.arange(D)[None, :]), terms)   # one fp32 addition after the other, in `order`
    if c.dcls:
        skip = (~kept).reshape(c.B, c.T) if wrong == "dcls_skips_dropped" else None
        emu_colsum(dX, ins["classes"].numpy(), out["dcls"].numpy(), c.T, D, c.s_off, c.S_out, c.alpha, skip=skip)
    return out


def emu_colsum_case(c, ins, wrong=None):
    out = K.colsum_outputs(c)
    emu_colsum(ins["X"].float().numpy(), ins["idx"].numpy(), out["dst"].numpy(), c.T, c.D, c.s_off, c.S_out, c.alpha, wrong)
    return out


def emu_mask(c, wrong=None):
    i = np.arange(c.B * c.S)
    lim = c.lens.astype(np.int64)[i // c.S] + c.add
    return ((i % c.S) <= lim if wrong == "le" else (i % c.S) < lim).astype(np.uint8).reshape(c.B, c.S)


def emu_seg(ins, wrong=None):
    """segment_sumsq_kernel's order in fp32: thread tid takes lo + tid, lo + tid + 256, ...; a butterfly per wave; four waves"""
    x = ins["x"].numpy()
    out = []
    for lo, hi in ins["ranges"].numpy():
        hi = hi + 1 if wrong == "end_inclusive" else hi
        acc = np.zeros(256, dtype=F32)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for base in range(lo, hi, 256):
                seg = x[base:min(base + 256, hi)]
                acc[:len(seg)] += seg * seg
            w = acc.reshape(4, 64)
            while w.shape[1] > 1:
                h = w.shape[1] // 2
                w = w[:, :h] + w[:, h:]
            out.append(F32(F32(F32(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]))
    return torch.from_numpy(np.array(out, dtype=F32))


def _ok(c, results):
    for r in results:
        assert not r.bad.any() and r.ratio <= 1.0, (c.id, r.name, int(r.bad.sum()), r.ratio)
    return ", ".join(f"{r.name} {r.ratio:.3f}" for r in results)


def _share(r, sel):
    assert sel.any()
    return float(r.bad[sel].mean())


# ------------------------------------------------------------------------------------------ the references are right
@pytest.mark.parametrize("c", K.EMBED_CASES, ids=lambda c: c.id)
def test_embed_reference_equals_torch_autograd(c):
    ins = K.embed_operands(c)
    D = c.D
    kept = torch.from_numpy(K._kept(c, ins)).double()
    tok = ins["tokens"].reshape(-1).long()
    if c.nan_row:   # what the contract rests on: the NaN row is referenced by dropped positions only
        assert (tok == K.NAN_TOKEN).any() and not (kept.bool() & (tok == K.NAN_TOKEN)).any() and ins["table"][K.NAN_TOKEN].isnan().all()
    table = torch.nan_to_num(ins["table"][:, :D].double(), nan=0.0).requires_grad_(True)
    leaves = [table]
    x = table[tok] * kept[:, None]
    if c.cls:
        cls = ins["cls_table"][:, :D].double().clone().requires_grad_(True)
        leaves.append(cls)
        x = x + cls[ins["classes"].long().repeat_interleave(c.T)]
    t = torch.arange(c.B * c.T) % c.T
    y = c.alpha * x + ins["pos"][c.s_off + t, :D].double()
    rows_ = torch.from_numpy(K.embed_rows(c))
    if c.fwd:
        got = K.embed_fwd_outputs(c)
        res = K.embed_fwd_check(c, ins, got)
        assert np.abs(res[0].ref - y.detach().numpy()).max() <= 1e-12 * max(1.0, float(y.detach().abs().max()))
        assert np.isfinite(res[0].ref).all() and np.isfinite(res[0].bound).all()
        if c.keymask:
            assert (res[1].ref == (tok != 0).numpy()).all() and (res[1].bound == 0).all()
        if c.nan_row:   # the header's "the table row is not read": alpha cls + pos, finite
            d = (tok == K.NAN_TOKEN).numpy()
            cc = ins["cls_table"][:, :D].double().numpy()[ins["classes"].numpy()[np.arange(c.B * c.T) // c.T]]
            want = c.alpha * cc[d] + ins["pos"][c.s_off + t, :D].double().numpy()[d]
            assert np.abs(res[0].ref[d] - want).max() <= 1e-12 * np.abs(want).max()
    up = ins["dX"][rows_, :D].double()
    grads = torch.autograd.grad(y, leaves, up)
    before = K.embed_bwd_outputs(c)
    res = K.embed_bwd_check(c, ins, before, before)
    assert len(res) == (2 if c.dcls else 1)
    want = before["dtable"][:K.V, :D].double() + grads[0]
    assert np.abs(res[0].ref - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))
    if c.dcls:
        want = before["dcls"][:K.NCLS, :D].double() + grads[1]
        assert np.abs(res[1].ref - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))
    untouched = np.bincount(tok[kept.bool()].numpy(), minlength=K.V) == 0
    assert (res[0].bound[untouched] == 0).all() and (res[0].bound[~untouched] > 0).all()


def test_colsum_mask_and_segment_references_on_hand_worked_answers():
    # colsum: two samples of class 1, one of class 0; T = 2 of S_out = 4 rows from row 1; alpha = 2; initial values 10, 20, 30
    X = np.arange(3 * 4 * 2, dtype=np.float64).reshape(12, 2)   # row r holds (2 r, 2 r + 1)
    ref, bound = K.colsum_ref(X, np.array([1, 0, 1]), 3, 2, 1, 4, 2.0, np.array([[10.0, 10], [20, 20], [30, 30]]))
    # sample 0: rows 1, 2 -> (2 + 4, 3 + 5); sample 1: rows 5, 6 -> (10 + 12, 11 + 13); sample 2: rows 9, 10 -> (18 + 20, 19 + 21)
    assert ref.tolist() == [[10 + 2 * 22, 10 + 2 * 24], [20 + 2 * (6 + 38), 20 + 2 * (8 + 40)], [30, 30]]
    assert (bound[2] == 0).all() and np.allclose(bound[0], K.gamma(4) * (10 + 2 * np.array([22.0, 24])), rtol=1e-12)
    assert np.allclose(bound[1], K.gamma(6) * (20 + 2 * np.array([44.0, 48])), rtol=1e-12)
    # mask
    c = K.Mask(5, 51, -1)
    assert c.lens.tolist() == [1, 50, 51, 54, 0]
    want = [[1 if s < n else 0 for s in range(51)] for n in (0, 49, 50, 53, -1)]
    assert K.mask_ref(c).tolist() == want and sum(want[4]) == 0 and sum(want[3]) == 51 and sum(want[2]) == 50
    for c in K.MASK_CASES:
        m = K.mask_ref(c)
        for b in range(c.B):
            assert int(m[b].sum()) == min(max(int(c.lens[b]) + c.add, 0), c.S) and (np.diff(m[b].astype(int)) <= 0).all()
    # segments
    for c in K.SEG_CASES:
        ins = K.seg_operands(c)
        x = ins["x"].double().tolist()
        r, g_inf, w_inf = K.seg_check(ins, torch.zeros(c.n))
        fs = [math.fsum(v * v for v in x[a:b]) for a, b in ins["ranges"].tolist()]
        fin = [v for v in fs if math.isfinite(v)]
        assert np.allclose(r.ref, fin, rtol=1e-13, atol=0) and len(w_inf) == len(fs) - len(fin)
        assert (r.bound[r.ref > 0] < 1e-3 * r.ref[r.ref > 0]).all(), "the bound stays a small share of the sum"
        if c.n == 300:
            assert len(w_inf) == 1 and np.isinf(w_inf).all() and r.ref[0] < 1e38 and r.ref[0] > 1e35 and r.ref[1] == 0 and r.bound[1] == 0  # (the inf segment is not among r's)
            xs = np.abs(ins["x"].numpy()[K.SEG_WIDE[0]:K.SEG_WIDE[1]])
            assert xs.min() <= 1e-20 and xs.max() >= 1e18 and np.isfinite(ins["x"].numpy()[:K.SEG_INF[0]]).all()


# ------------------------------------------------------------------------------------------ the tables reach what they are meant for
def test_the_embedding_table_is_complete():
    for dt in K.DTYPES:
        cs = [c for c in K.EMBED_CASES if c.dtype == dt]
        fwd = [c for c in cs if c.fwd]
        assert {c.D for c in fwd} == {4, 8, 40, 256, 260, 1024} and {c.s_off for c in fwd} == {0, 1}
        assert any(c.B * c.T == 16387 and c.D == 8 for c in fwd), "a second trip of the grid-stride loop (4096 workgroups of 4 rows)"
        assert any(c.extra > 0 and c.s_off > 0 for c in fwd) and {c.pad for c in fwd} == {True, False}
        assert {c.cls for c in fwd} == {True, False} and {c.keymask for c in fwd} == {True, False}
        assert any(c.keep and c.cls for c in fwd) and any(c.keep is None for c in fwd) and any(c.nan_row and c.cls for c in fwd)
        assert any(c.keep == "sample" and c.dcls for c in cs) and any(c.tokens == "equal" and c.B * c.T >= 512 for c in cs)
        assert {c.D for c in cs if not c.dcls} >= {4, 12} and any(c.dcls and c.B * c.T > 16384 for c in cs)
        for c in cs:
            ins = K.embed_operands(c)
            tok = ins["tokens"].numpy()
            if c.tokens == "mixed":
                assert (tok == 0).any() and (tok == K.V - 1).any() and (tok[-1] == tok[-1, 0]).all()
            if c.tokens == "runs":
                assert max(len(s) for s in "".join("x" if a == b else " " for a, b in zip(tok.reshape(-1)[1:], tok.reshape(-1)[:-1])).split()) >= 299
            assert set(ins["classes"].tolist()) <= {0, 2}
            if c.keep == "sample":
                assert ins["keep"].view(c.B, c.T)[1].sum() == 0 and ins["keep"].sum() > 0
            if c.pad:
                assert ins["table"].stride(0) > c.D and ins["pos"].stride(0) > c.D and ins["dX"].stride(0) > c.D
                assert ins["table"][:, c.D:].isnan().all() and ins["dX"][:, c.D:].isnan().all()
            own = np.zeros(c.B * c.S_out + K.GUARD, dtype=bool)
            own[K.embed_rows(c)] = True
            assert ins["dX"][torch.from_numpy(~own)].isnan().all() and ins["dX"][torch.from_numpy(own), :c.D].isfinite().all()
    assert len({c.id for c in K.EMBED_CASES}) == len(K.EMBED_CASES)


def test_the_colsum_table_reaches_every_edge_of_the_thread_map(ops):
    """the thread map asked of the library (mst_group_colsum_form: no HIP call)"""
    for c in K.COLSUM_CASES:
        q = ops.group_colsum_form(c.T, c.D)
        assert (q["cpr"], q["rg"], q["grid"], q["lds"]) == c.form, c.id
        assert q["lds"] <= 8192
    for dt in K.DTYPES:
        cs = [c for c in K.COLSUM_CASES if c.dtype == dt]
        assert {(c.D, c.T) for c in cs} == {(D, T) for D in K.COLSUM_D for T in K.COLSUM_T}
        forms = {c.form[:2] for c in cs}
        assert any(cpr * rg < 256 for cpr, rg in forms), "idle threads"
        assert any(rg == 1 and cpr < 256 for cpr, rg in forms) and (256, 1) in forms and (1, 256) in forms
        assert {c.s_off for c in cs} == {0, 1} and {c.pad for c in cs} == {True, False} and {c.one_class for c in cs} == {True, False}
        assert any(c.alpha != 1 for c in cs) and any(c.extra > 0 for c in cs)
        for c in cs:
            assert 1 not in K.colsum_operands(c)["idx"].tolist()
    assert len({c.id for c in K.COLSUM_CASES}) == len(K.COLSUM_CASES)
    with pytest.raises(ops._lib.MstError, match="multiple of 8"):
        ops.group_colsum_form(4, 12)


def test_the_mask_and_segment_tables_are_complete():
    assert {c.B * c.S for c in K.MASK_CASES} == {255, 256, 257, 3 * 256 + 1} and {c.add for c in K.MASK_CASES} == {-1, 0, 1}
    rel = set()
    for c in K.MASK_CASES:
        rel |= {int(n) - c.S for n in c.lens if n > 1} | {int(n) for n in c.lens if n <= 1}
    assert rel >= {0, 1, -1, 3}, "lens of 0, 1, S - 1, S, S + 3"
    assert any((c.lens.astype(int) + c.add < 0).any() for c in K.MASK_CASES)
    assert {c.n for c in K.SEG_CASES} == {1, 300}
    r = K.seg_operands(K.Seg(300))["ranges"].numpy()
    assert len(r) == 300 and {0, 1, 255, 256, 257, 5000} <= set((r[:, 1] - r[:, 0]).tolist()) and (r[:, 0] % 4 != 0).any()
    assert any(a < d and c < b for (a, b) in r[:12] for (c, d) in r[:12] if (a, b) != (c, d)), "overlapping ranges"
    assert r.max() <= K.SEG_N


# ------------------------------------------------------------------------------------------ the bounds take an fp32 evaluation
@pytest.mark.parametrize("c", EMBED_FWD, ids=lambda c: c.id)
def test_embed_fwd_bound_takes_fp32_fused_or_not(c):
    ins = K.embed_operands(c)
    for fused in (False, True):
        out = emu_embed_fwd(c, ins, fused=fused)
        print(f"\n{c.id} fused={fused}: worst fp32 error / bound " + _ok(c, K.embed_fwd_check(c, ins, out)))
        assert K.embed_fwd_intact(c, out) == []
    r = K.embed_fwd_check(c, ins, out)[0]
    assert np.median(r.bound) < 0.01 * np.abs(r.ref).max()


@pytest.mark.parametrize("c", K.EMBED_CASES, ids=lambda c: c.id)
def test_embed_bwd_bound_takes_fp32_in_two_orders(c):
    ins = K.embed_operands(c)
    before = K.embed_bwd_outputs(c)
    for reverse in (False, True):
        out = emu_embed_bwd(c, ins, reverse=reverse)
        res = K.embed_bwd_check(c, ins, before, out)
        print(f"\n{c.id} reverse={reverse}: worst fp32 error / bound " + _ok(c, res))
        assert K.embed_bwd_intact(c, out) == []
    for r in res:  # (a worst-case bound over n terms against a sum that grows as sqrt(n): 3 % of it at the 9364 terms of the largest case)
        assert np.median(r.bound) < 0.05 * np.abs(r.ref).max()


@pytest.mark.parametrize("c", K.COLSUM_CASES, ids=lambda c: c.id)
def test_colsum_bound_takes_the_kernels_thread_map_in_fp32(c):
    ins = K.colsum_operands(c)
    out = emu_colsum_case(c, ins)
    res = K.colsum_check(c, ins, K.colsum_outputs(c), out)
    print(f"\n{c.id}: worst fp32 error / bound " + _ok(c, res))
    assert K.intact2d("dst", out["dst"], np.arange(K.NCLS), c.D) == []
    assert (res[0].bound[1] == 0).all() and (res[0].got[1] == res[0].ref[1]).all(), "the class nobody is in keeps its values"


def test_mask_and_segment_emulations_are_accepted():
    for c in K.MASK_CASES:
        assert (emu_mask(c) == K.mask_ref(c)).all()
    for c in K.SEG_CASES:
        ins = K.seg_operands(c)
        r, g_inf, w_inf = K.seg_check(ins, emu_seg(ins))
        assert not r.bad.any() and r.ratio <= 1.0 and (g_inf == w_inf).all()
        print(f"\n{c.id}: worst fp32 error / bound {r.ratio:.3f}")


# ------------------------------------------------------------------------------------------ the bounds refuse what they must
@pytest.mark.parametrize("dtype", K.DTYPES, ids=lambda d: K.DT_NAME[d])
def test_the_bounds_refuse_wrong_embedding_kernels(dtype):
    seen = set()
    for c in (c for c in K.EMBED_CASES if c.dtype == dtype):
        ins = K.embed_operands(c)
        kept = K._kept(c, ins)
        tok = ins["tokens"].numpy().reshape(-1)
        allD = lambda rows_: np.broadcast_to(rows_[:, None], (c.B * c.T, c.D))  # noqa: E731
        if c.fwd and c.s_off:
            # another row of pos (or NaN from a row outside the launch): unit-scale values against half an ulp
            r = K.embed_fwd_check(c, ins, emu_embed_fwd(c, ins, "pos_row_t"))[0]
            assert _share(r, allD(np.ones(c.B * c.T, dtype=bool))) >= 0.95, c.id
            seen.add("pos_row_t")
        if c.fwd and c.cls:
            b = np.arange(c.B * c.T) // c.T
            cl = ins["classes"].numpy()
            differ = cl[np.arange(c.B * c.T) % c.B] != cl[b]
            if differ.any():
                r = K.embed_fwd_check(c, ins, emu_embed_fwd(c, ins, "class_of_row"))[0]
                assert _share(r, allD(differ)) >= 0.95, c.id
                seen.add("class_of_row")
        if c.fwd and c.keymask and c.keep:
            differ = kept != (tok != 0)
            r = K.embed_fwd_check(c, ins, emu_embed_fwd(c, ins, "keymask_from_keep"))[1]
            assert _share(r, differ) == 1.0, c.id
            seen.add("keymask_from_keep")
        if c.keep:
            before = K.embed_bwd_outputs(c)
            r = K.embed_bwd_check(c, ins, before, emu_embed_bwd(c, ins, "dropped_scattered"))[0]
            hit = np.bincount(tok[~kept], minlength=K.V) > 0
            # a whole extra term alpha dX of unit scale against gamma_(n + 1) of the sum
            assert _share(r, np.broadcast_to(hit[:, None], (K.V, c.D))) >= 0.95, c.id
            seen.add("dropped_scattered")
            if c.dcls:
                r = K.embed_bwd_check(c, ins, before, emu_embed_bwd(c, ins, "dcls_skips_dropped"))[1]
                used = np.bincount(ins["classes"].numpy()[(np.arange(c.B * c.T) // c.T)[~kept]], minlength=K.NCLS) > 0
                # the missing terms sum to a normal deviate of sigma = alpha 0.5 sqrt(dropped frames of the class) against a worst-case
                # bound of gamma_(n + 2) over all n: outside it with probability erfc(bound / (sigma sqrt 2)), which is 1 in the
                # small cases and 0.94 at 9364 frames per class (16 elements there: a share of 0.06 more or less is chance)
                nd = np.bincount(ins["classes"].numpy()[(np.arange(c.B * c.T) // c.T)[~kept]], minlength=K.NCLS)[used].min()
                expect = math.erfc(float(r.bound[used].max()) / (c.alpha * 0.5 * math.sqrt(nd) * math.sqrt(2)))
                assert _share(r, np.broadcast_to(used[:, None], (K.NCLS, c.D))) >= expect - 0.2, (c.id, expect)
                seen.add("dcls_skips_dropped")
    assert seen == {"pos_row_t", "class_of_row", "keymask_from_keep", "dropped_scattered", "dcls_skips_dropped"}


def test_the_bounds_refuse_wrong_reductions_and_masks():
    n_clip = n_off = 0
    for c in K.COLSUM_CASES:
        ins = K.colsum_operands(c)
        before = K.colsum_outputs(c)
        used = np.zeros((K.NCLS, c.D), dtype=bool)
        used[ins["idx"].numpy()] = True
        if c.T % 64:
            # frames behind T: the next sample's, or NaN (rows the launch does not own) -> every column of every class in use
            r = K.colsum_check(c, ins, before, emu_colsum_case(c, ins, "chunk_not_clipped"))[0]
            assert _share(r, used) >= 0.95, c.id
            n_clip += 1
        if c.s_off:
            r = K.colsum_check(c, ins, before, emu_colsum_case(c, ins, "s_off_ignored"))[0]
            assert _share(r, used) >= 0.95, c.id
            n_off += 1
    assert n_clip >= 40 and n_off >= 20
    for c in K.MASK_CASES:
        lim = c.lens.astype(int) + c.add
        wrong, ref = emu_mask(c, "le"), K.mask_ref(c)
        rows_ = (lim >= 0) & (lim < c.S)   # where position `lim` exists it is the one that differs
        assert (wrong[rows_, lim[rows_]] != ref[rows_, lim[rows_]]).all()
        assert rows_.any() or c.B == 1
    assert sum(((c.lens.astype(int) + c.add >= 0) & (c.lens.astype(int) + c.add < c.S)).sum() for c in K.MASK_CASES) >= 10
    ins = K.seg_operands(K.Seg(300))
    r, _, _ = K.seg_check(ins, emu_seg(ins, "end_inclusive"))
    x = ins["x"].double().numpy()
    fin = np.array([np.isfinite((x[a:b] ** 2).sum()) for a, b in ins["ranges"].numpy()])
    extra = x[ins["ranges"].numpy()[fin, 1]] ** 2   # the element behind the range (NaN behind the last one)
    big = ~(extra <= 2 * r.bound)                   # one more square: seen wherever it is larger than the bound it is held to
    assert big.sum() >= 200 and r.bad[big].all()


# ------------------------------------------------------------------------------------------ refusals: status and message, no launch
ONE = 4096   # a non-NULL, 16-byte aligned stand-in for a device buffer: a refused call follows no pointer


@pytest.mark.parametrize("entry, changes, status, fragment", K.REFUSALS, ids=[f"{e}-{'-'.join(f'{k}={v}' for k, v in ch.items())}" for e, ch, _, _ in K.REFUSALS])
def test_every_refusal_comes_before_any_launch(ops, entry, changes, status, fragment):
    lib = ops._lib.load()
    form = (C.c_int64 * 4)()
    ptrs = {name: ONE for name in K.POINTERS}
    ptrs["form"] = C.addressof(form)
    args = K.refusal_args(entry, changes, ptrs)
    assert getattr(lib, entry)(*args) == status
    assert fragment.encode() in lib.mst_last_error(), lib.mst_last_error()


def test_the_refusal_list_covers_every_check_of_the_sources():
    """every MST_CHECK_ARG message of the entry points in csrc/embed.hip and of mst_segment_sumsq appears in the list"""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musicstyletransfer_amd", "csrc")
    text = open(os.path.join(root, "embed.hip")).read()
    optim = open(os.path.join(root, "optim.hip")).read()
    text += optim[optim.index('extern "C" int mst_segment_sumsq'):optim.index('extern "C" int mst_cast_f32_to_act')]
    msgs = re.findall(r'MST_CHECK_ARG\((?:[^"]|\n)*?"([^"]+)"', text)
    assert len(msgs) >= 14
    frags = [f for _, _, _, f in K.REFUSALS]
    for m in set(msgs):
        assert any(f and f in m for f in frags), m
