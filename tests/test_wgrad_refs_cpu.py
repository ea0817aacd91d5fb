"""mst_gemm_wgrad_batch_flush without a GPU: the batches of tests/wgrad_refs.py get the plan they record (asked of
mst_gemm_wgrad_plan, the flush's own decision) and between them reach every launch form, body, slab kind, remap kind and scratch
outcome; the plan's boundaries sit where the header says; and the derived tolerance accepts a correct fp32 evaluation and refuses
the wrong results a weight-gradient kernel is prone to (a dropped row, a remap off by a row)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_refs as W  # noqa: E402
from wgrad_refs import Prob  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def plan_of(probs, scratch_bytes=0, dtype=W.BF, **over):
    from musicstyletransfer_amd import _lib, ops
    return ops.gemm_wgrad_plan(W.plan_args(probs, dtype, _lib.WgradArgs, **over), scratch_bytes)


def P(M, N, K, **kw):
    return Prob("edge", M, N, K, **kw)


# ------------------------------------------------------------------------------------------ the cases get their plans
def test_abi_104_exports_the_plan_query(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 104
    assert len(_lib.SIGNATURES["mst_gemm_wgrad_plan"][1]) == 4


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_every_case_gets_the_plan_it_records(lib, case):
    """fails when a threshold or the split rule moves and a batch silently runs another kernel"""
    got = plan_of(case.probs, case.scratch_bytes, case.dtype)
    assert got == W.plan_dict(case.plan), case.id
    # the recorded items and the output range, restated
    plan, total = case.plan, sum(p.N * p.K for p in case.probs)
    lo = 0 if plan.form == 0 else W.THRESHOLDS[plan.form - 1]
    hi = W.THRESHOLDS[plan.form] if plan.form < 3 else lo + 256 * 256  # form 3: close to its threshold
    assert lo <= total < hi
    assert all(p.M <= 520 for p in case.probs) and len(case.probs) <= 16
    assert plan.items == sum(W.tiles(p, plan.form, (plan.narrow >> i) & 1) * s for i, (p, s) in enumerate(zip(case.probs, plan.splits)))
    assert plan.items <= W.SLOTS[plan.form]
    assert case.scratch_bytes < 48 << 20


def test_the_cases_reach_every_form_body_slab_remap_and_scratch_outcome(lib):
    bodies, slabs, remaps, scratch = set(), set(), set(), set()
    for c in W.CASES:
        plan = plan_of(c.probs, c.scratch_bytes, c.dtype)
        scratch.add((c.scratch, plan["two_pass"]))
        for i, (p, split) in enumerate(zip(c.probs, plan["splits"])):
            narrow = (plan["narrow"] >> i) & 1
            assert narrow == (plan["form"] == 3 and p.K <= 128)
            whole = W.whole_stages(p.M, split)
            # which kinds end in a ragged slab is a property of their M: 500, 264 (8 x 33), 520 and 40 do, 512 and 64 do not
            assert whole == (p.M % 64 == 0), (c.id, p.kind)
            assert sum(W.slab_rows(p.M, split)) == p.M
            bodies.add((c.dtype, plan["form"], p.body(narrow)))
            slabs.add((c.dtype, plan["form"], "whole" if whole else "ragged"))
            # (the interleaved main loop: whole-stage slabs and no divided remap)
            slabs.add((c.dtype, plan["form"], "interleaved" if whole and p.remap_kind != "divided" else "fallback"))
            remaps.add((c.dtype, plan["form"], p.remap_kind))
    for d in W.DTYPES:
        for f in range(4):
            for b in ("16", "u8") + (("narrow-16", "narrow-u8") if f == 3 else ()):
                assert (d, f, b) in bodies, (f, b)
            for s in ("whole", "ragged", "interleaved", "fallback"):
                assert (d, f, s) in slabs, (f, s)
            for r in ("none", "carried", "divided", "b-only"):
                assert (d, f, r) in remaps, (f, r)
    assert len(bodies) == 2 * (2 * 4 + 2)
    assert scratch == {("none", 0), ("both", 3), ("tiles", 1), ("small", 0)}
    # a remap group of exactly 64 rows (carried, not divided) in every form, on A alone
    assert all(any(p.ta == 64 and not p.tb for p in W.BATCHES[f]) for f in range(4))


def test_case_ids_are_unique_and_operands_match_the_layout():
    assert len({c.id for c in W.CASES}) == len(W.CASES) == 2 * (3 + 4)
    ops_ = W.operands(0, W.BF, "real")
    for p, o in zip(W.BATCHES[0], ops_):
        assert o["A"].shape == (p.rows(p.ta), p.lda) and o["B"].shape == (p.rows(p.tb), p.ldb)
        assert o["A"].dtype == (torch.uint8 if p.a_u8 else W.BF)
        if not p.a_u8:
            a = o["A"].float()
            assert torch.isfinite(a[torch.from_numpy(p.phys(p.ta)), :W.roundup(p.N, 8)]).all()
            assert (a[torch.from_numpy(p.phys(p.ta)), p.N:W.roundup(p.N, 8)] == 0).all()
            assert not p.pad or torch.isnan(a[:, W.roundup(p.N, 8):]).all()
            assert not p.ta or torch.isnan(a[::p.ta + 1]).all()
        else:
            assert set(np.unique(o["A"].numpy())) == set(range(7)) and (o["A"][:, p.N:] == 0).all()
        b = o["B"].float()
        assert not p.tb or torch.isnan(b[::p.tb + 1]).all()
    p = W.BATCHES[0][2]
    assert p.phys(128)[:2].tolist() == [1, 2] and p.phys(128)[128] == 130
    assert W.slab_rows(264, 3) == [128, 128, 8] and W.slab_rows(512, 3) == [192, 192, 128] and W.slab_rows(64, 4) == [64]


# ------------------------------------------------------------------------------------------ plan edges
@pytest.mark.parametrize("form", (1, 2, 3))
def test_output_size_thresholds(lib, form):
    thr = W.THRESHOLDS[form - 1]
    assert plan_of([P(256, 1, thr - 1)])["form"] == form - 1
    assert plan_of([P(256, 1, thr)])["form"] == form
    # the total of the batch decides, not a problem's own size
    assert plan_of([P(256, 1, thr - 64), P(256, 8, 8)])["form"] == form
    assert plan_of([P(256, 1, thr - 64), P(256, 7, 9)])["form"] == form - 1


def test_narrow_body_at_k_128(lib):
    big = P(512, 1536, 1024)
    assert plan_of([big, P(512, 256, 128)])["narrow"] == 0b10
    assert plan_of([big, P(512, 256, 136)])["narrow"] == 0
    assert plan_of([P(512, 256, 72), big, P(512, 256, 128, a_u8=True)])["narrow"] == 0b101
    # no narrow body outside form 3
    pl = plan_of([P(512, 1152, 1024), P(512, 256, 128)])
    assert (pl["form"], pl["narrow"]) == (2, 0)


def test_splits(lib):
    # a 64-row problem gets one slab inside a batch that is split
    assert plan_of([P(512, 64, 64), P(64, 64, 64), P(129, 64, 64), P(128, 64, 64)])["splits"] == [4, 1, 2, 1]
    # form 3, 24 wide tiles and one narrow: 24 S + (5 S + 4) / 8 <= 256 holds up to S = 10; the narrow split is (5 S + 4) / 8 = 6,
    # capped by cdiv(M, 128)
    big = P(2048, 1536, 1024)
    pl = plan_of([big, P(2048, 256, 128)])
    assert (pl["form"], pl["narrow"], pl["splits"], pl["items"]) == (3, 0b10, [10, 6], 246)
    pl = plan_of([big, P(2048, 256, 128), P(512, 256, 128), P(64, 256, 72)])
    assert (pl["splits"], pl["items"]) == ([10, 6, 4, 1], 251)


@pytest.mark.parametrize("form,M,fits,over", [
    # (tiles, split, items) each side of the resident round: S is the largest split at which the items still fit
    (0, 8192, (16, 64, 1024), (17, 60, 1020)),
    (1, 2048, (32, 16, 512), (33, 15, 495)),
    (2, 1024, (42, 6, 252), (43, 5, 215)),
    (3, 1024, (32, 8, 256), (33, 7, 231)),
])
def test_items_fill_one_resident_round(lib, form, M, fits, over):
    bn, bk = W.TILE[form]
    for tiles, split, items in (fits, over):
        pl = plan_of([P(M, bn * tiles, bk)])
        assert (pl["form"], pl["splits"], pl["items"]) == (form, [split], items)
        assert items <= W.SLOTS[form] < tiles * (split + 1)


def test_scratch_outcomes_at_their_byte_boundaries(lib):
    probs = [P(1024, 8192, 256)]
    n = plan_of(probs)["items"]
    assert n == 256
    assert plan_of(probs, n * W.SLOT_BYTES - 1)["two_pass"] == 0
    assert plan_of(probs, n * W.SLOT_BYTES)["two_pass"] == 1
    assert plan_of(probs, n * (W.SLOT_BYTES + W.BIAS_ROW_BYTES) - 1)["two_pass"] == 1
    assert plan_of(probs, n * (W.SLOT_BYTES + W.BIAS_ROW_BYTES))["two_pass"] == 3
    # only the 256 x 256 form has a reduction pass
    for f in range(3):
        assert plan_of(W.BATCHES[f], 1 << 30)["two_pass"] == 0
    # the scratch buffer changes nothing else
    a, b = plan_of(W.BATCHES[3]), plan_of(W.BATCHES[3], 1 << 30)
    assert b.pop("two_pass") == 3 and a.pop("two_pass") == 0 and a == b


@pytest.mark.parametrize("n,over,text", [
    (0, {}, b"need 1..16 problems"), (17, {}, b"need 1..16 problems"),
    (2, dict(lda=64), b"lda/ldb must be"), (2, dict(ldw=60), b"ldw < K"), (2, dict(A=4104), b"16-byte aligned"),
    (2, dict(M=1 << 30), b"below 2^30"), (2, dict(B=None), b"null operand"), (2, dict(K=0), b"must be positive"),
])
def test_the_plan_query_rejects_what_the_flush_rejects(lib, n, over, text):
    """validation comes before any HIP call in both: same status, same message"""
    from musicstyletransfer_amd import _lib
    args = W.plan_args([P(256, 72, 64)] * max(n, 1), W.BF, _lib.WgradArgs, **over)
    arr = (_lib.WgradArgs * len(args))(*args)
    plan = (ctypes.c_int64 * 20)()
    rc = lib.mst_gemm_wgrad_plan(arr, n, 0, plan)
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg, (rc, msg)
    assert lib.mst_gemm_wgrad_batch_flush(arr, n, None, 0, None, 0, None, 0, None) == -1 and lib.mst_last_error() == msg


def test_the_plan_query_rejects_mixed_and_unknown_dtypes(lib):
    from musicstyletransfer_amd import _lib
    plan = (ctypes.c_int64 * 20)()
    for dtypes, rc_want, text in (((0, 1), -1, b"mixed dtypes"), ((2, 2), -3, b"unsupported activation dtype")):
        args = W.plan_args([P(256, 72, 64)] * 2, W.BF, _lib.WgradArgs)
        args[0].dtype, args[1].dtype = dtypes
        arr = (_lib.WgradArgs * 2)(*args)
        assert lib.mst_gemm_wgrad_plan(arr, 2, 0, plan) == rc_want and text in lib.mst_last_error()
        msg = lib.mst_last_error()
        assert lib.mst_gemm_wgrad_batch_flush(arr, 2, None, 0, None, 0, None, 0, None) == rc_want and lib.mst_last_error() == msg
    assert lib.mst_gemm_wgrad_plan(None, 1, 0, plan) == -1 and lib.mst_gemm_wgrad_plan(arr, 2, 0, None) == -1
    with pytest.raises(_lib.MstError, match="ldw < K"):
        plan_of([P(256, 72, 64)], ldw=8)


# ------------------------------------------------------------------------------------------ the reference and its bound
def fp32_eval(p, o):
    """the operation in fp32 torch on the CPU -> (dW, db) fp64"""
    A, B = (torch.from_numpy(x).float() for x in W.gathered(p, o))
    s = torch.tensor(p.scale, dtype=torch.float32)
    dW = torch.from_numpy(o["dW0"]).float() + s * (A.t() @ B)
    db = torch.from_numpy(o["db0"]).float() + (s * A.sum(0) if p.db else 0.0)
    return dW.double().numpy(), db.double().numpy()


def zeroed(o):
    """the operands with the poison replaced by zeros: what a remap that is off by a row then gathers"""
    return dict(o, A=o["A"] if o["A"].dtype == torch.uint8 else torch.nan_to_num(o["A"].float()).to(o["A"].dtype),
                B=torch.nan_to_num(o["B"].float()).to(o["B"].dtype))


def shifted(p):
    """a remap's offset moved by a row, on A where A is remapped, else on B"""
    return dict(a_shift=-1) if p.ta else dict(b_shift=-1)


@pytest.mark.parametrize("dtype", W.DTYPES, ids=lambda d: W.DT_NAME[d])
@pytest.mark.parametrize("form", range(4))
def test_the_bound_takes_fp32_and_refuses_a_dropped_row_and_a_shifted_remap(form, dtype):
    for i, (p, o, r) in enumerate(zip(W.BATCHES[form], W.operands(form, dtype, "real"), W.references(form, dtype, "real"))):
        what = f"form {form} problem {i} ({p.kind})"
        assert np.isfinite(r["dW"]).all() and np.isfinite(r["db"]).all(), what
        bW, bb = W.wgrad_bound(p.M, r["dW"], r["SW"]), W.wgrad_bound(p.M, r["db"], r["Sb"])
        dW, db = fp32_eval(p, o)
        assert (np.abs(dW - r["dW"]) <= bW).all() and (np.abs(db - r["db"]) <= bb).all(), f"{what}: fp32 outside the bound"
        assert np.median(bW) < 0.02 * np.median(np.abs(r["dW"] - o["dW0"])), f"{what}: a bound of the size of the result would accept anything"
        if p.a_u8:
            continue
        # one logical row left out of the sum: at least half of the problem's elements must leave the bound
        for row in (0, p.M // 2, p.M - 1):
            w = W.wgrad_ref(p, o, drop_row=row)
            frac = (np.abs(w["dW"] - r["dW"]) > bW).mean()
            assert frac >= 0.5, f"{what}: a dropped row {row} leaves the bound at {frac:.0%} of the elements only"
            assert not p.db or (np.abs(w["db"] - r["db"]) > bb).mean() >= 0.5, what
        if p.ta or p.tb:
            w = W.wgrad_ref(p, zeroed(o), **shifted(p))
            frac = (np.abs(w["dW"] - r["dW"]) > bW).mean()
            assert frac >= 0.5, f"{what}: a remap off by a row leaves the bound at {frac:.0%} of the elements only"


@pytest.mark.parametrize("dtype", W.DTYPES, ids=lambda d: W.DT_NAME[d])
@pytest.mark.parametrize("form", range(4))
def test_integer_mode_is_exact_in_fp32_and_sees_the_same_mutations(form, dtype):
    for i, (p, o, r) in enumerate(zip(W.BATCHES[form], W.operands(form, dtype, "int"), W.references(form, dtype, "int"))):
        what = f"form {form} problem {i} ({p.kind})"
        # integers of fewer than 24 bits however the sum is ordered: |dW| <= 2 + 2 * 520 * 6 * 2
        assert np.array_equal(r["dW"], np.round(r["dW"] * 2) / 2) and np.abs(r["SW"]).max() + 2 < 2 ** 15, what
        dW, db = fp32_eval(p, o)
        assert np.array_equal(dW, r["dW"]) and np.array_equal(db, r["db"]), what
        w = W.wgrad_ref(p, o, drop_row=p.M // 2)
        assert not np.array_equal(w["dW"], r["dW"]), what
        if p.ta or p.tb:
            assert not np.array_equal(W.wgrad_ref(p, zeroed(o), **shifted(p))["dW"], r["dW"]), what


def test_rider_references_are_exact_integers():
    for d in W.DTYPES:
        sums, outers = W.rider_refs(W.rider_operands(d))
        assert [s.shape for s in sums] == [(256,), (128,), (60,)] and [x.shape for x in outers] == [(24, 40), (16, 40), (16,)]
        assert all(np.array_equal(x, np.round(x)) and np.abs(x).max() < 2 ** 20 for x in sums + outers)
