"""tests/attn_refs.py without a GPU: the fp64 reference against torch autograd and against answers worked out by hand, the case table
against the library's own launch decision (mst_attn_fwd_form / mst_attn_bwd_form) and against its restatement, the dispatch edges,
and the derived tolerance — it accepts an emulation that rounds where the kernels round and refuses every wrong result listed in
attn_refs.MUTATIONS."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_refs as A  # noqa: E402

BF, FP = A.BF, A.FP


@pytest.fixture(scope="module")
def ops():
    from musicstyletransfer_amd import _lib, ops as o
    _lib.load()
    return o


def _forms(o, c, monkeypatch, dtype=BF):
    if c.force:
        monkeypatch.setenv("MST_ATTN_PATH", c.force)
    else:
        monkeypatch.delenv("MST_ATTN_PATH", raising=False)
    fa, ba = A.form_calls(c, dtype)
    return o.attn_fwd_form(*fa), o.attn_bwd_form(*ba)


# ------------------------------------------------------------------------------------------ the reference itself
def _torch_attention(c, o, mode):
    """fp64 autograd on the flat qkv layout (its own indexing, not attn_refs.sections): the fp32 mask add emulated by a cast whose
    value replaces the fp64 logit while the gradient passes as the identity"""
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    qkv = torch.nan_to_num(o["qkv"].double(), nan=0.0).requires_grad_(True)
    x3 = qkv.view(B, S, -1)
    heads = lambda off: x3[:, :, off:off + D].reshape(B, S, H, dh).permute(0, 2, 1, 3)  # noqa: E731
    K, Q, V = (heads(off) for off in c.offs)
    scale = A.scale_of(dh)
    x = K @ Q.transpose(-1, -2)
    madd = torch.where(torch.from_numpy(c.valid(mode)).view(B, 1, S, 1), 0.0, A.MASK_VALUE).float()
    t32 = ((x.detach().float() * torch.tensor(scale, dtype=torch.float32)) + madd).double()
    t = x * scale + (t32 - x.detach() * scale)
    P = torch.softmax(t, dim=-1)
    out = (P.transpose(-1, -2) @ V).permute(0, 2, 1, 3)        # [B, S, H, dh]
    dO = torch.from_numpy(A.sections(c, o["qkv"].nan_to_num(0.0), o["dout"].nan_to_num(0.0))[3])
    ql = c.q_limit if 0 < c.q_limit < S else S
    (out[:, :ql] * dO[:, :ql]).sum().backward()
    g = qkv.grad.view(B, S, -1)
    dK, dQ, dV = (g[:, :, off:off + D].reshape(B, S, H, dh).numpy() for off in c.offs)
    lse = torch.logsumexp(t, dim=-1).detach().numpy()
    delta = (P * (V @ dO.permute(0, 2, 3, 1))).sum(-1).detach().numpy()   # sum_q P dP, dP[k, q] = V[k] . dO[q]
    return dict(out=out.detach().numpy(), lse=lse, dK=dK, dQ=dQ, dV=dV, delta=delta), ql


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("cid", ["d32-res3-s64", "d32-res3-s100-ql2", "d16-lone-s65-ql32", "d64-res3-s100", "d32-forced-s70"])
def test_reference_equals_torch_autograd_in_fp64(cid, mode):
    """padded rows of every kind, `big` inputs, q_limit and the permuted section offsets"""
    c = A.CASE[cid]
    o, r = A.operands(cid, BF, mode), A.references(cid, BF, mode)
    want, ql = _torch_attention(c, o, mode)
    for k in A.RESULTS:
        got, ref = r[k], want[k]
        if k == "out":
            assert not got[:, ql:].any()
            got, ref = got[:, :ql], ref[:, :ql]
        err = np.abs(got - ref).max()
        assert err <= 1e-9 * max(1.0, np.abs(ref).max()), f"{cid} {mode}: {k} off by {err}"


def test_an_all_padded_sequence_of_small_logits_gives_the_mean_of_v():
    """the header's quirk: the same -1e9 on a whole softmax row swallows every |x scale| < 32, the row is uniform"""
    rng = np.random.default_rng(3)
    S, dh = 37, 32
    K, Q, V, dO = (rng.standard_normal((S, dh)) for _ in range(4))
    r = A.head_ref(K, Q, V, np.zeros(S, dtype=bool), dO, 0, dh)
    assert np.allclose(r["out"], np.tile(V.mean(0), (S, 1)), rtol=0, atol=1e-13)
    assert np.array_equal(r["lse0"], np.full(S, -1e9)) and np.allclose(r["lse1"], np.log(S), rtol=0, atol=1e-13)
    assert np.allclose(r["dV"], np.tile(dO.mean(0), (S, 1)), rtol=0, atol=1e-13)


def test_a_big_padded_row_is_few_hot_as_worked_out_by_hand():
    """head size 16 (scale 1/4), padded key 0 = 100 e_0, queries with Q[q, 0] = 14, 12, 11, -3: x scale = 350, 300, 275, -75. fp32
    numbers near 1e9 are 64 apart and -1e9 is one of them, so t = -1e9 + 64 round(x scale / 64) = -1e9 + (320, 320, 256, -64): the row's
    maximum is -1e9 + 320, held by the first two queries, the third is e^-64 below, the fourth e^-384: P = (1/2, 1/2, ~0, ~0)."""
    rng = np.random.default_rng(4)
    S, dh = 4, 16
    K, Q, V, dO = (rng.integers(-3, 4, (S, dh)).astype(np.float64) for _ in range(4))
    K[0] = 0.0
    K[0, 0] = 100.0
    Q[:, 0] = (14, 12, 11, -3)
    valid = np.array([False, True, True, True])
    r = A.head_ref(K, Q, V, valid, dO, 0, dh)
    assert r["lse0"][0] == -1e9 + 320 and abs(r["lse1"][0] - np.log(2.0)) < 1e-15
    assert np.allclose(r["dV"][0], 0.5 * (dO[0] + dO[1]), rtol=0, atol=1e-13)
    # ... and were the row uniform (the fast form on a padded key), dV[0] would be the mean of all four
    assert np.abs(r["dV"][0] - dO.mean(0)).max() > 0.2
    assert np.allclose(A.head_ref(K, Q, V, valid, dO, 0, dh, mut="padded_uniform")["dV"][0], dO.mean(0), rtol=0, atol=1e-13)


def test_big_mode_keeps_every_padded_key_off_the_rounding_boundaries():
    """head sizes 16 and 64: scale is a power of two, x scale exact; head size 32: at least 0.5 from every boundary 32 + 64 n, where
    fl32(fl32(x scale) - 1e9) and fmaf(x, scale, -1e9) agree. And the padded rows really are not uniform."""
    assert len(A.good_multipliers()) >= 50
    spans = []
    for c in A.CASES:
        if c.fused:
            assert A.operands(c.id, BF, "big")["keymask"].all()
            continue
        if c.valid().all() or c.B * c.H > 64:
            continue
        for dtype in A.DTYPES:
            o = A.operands(c.id, dtype, "big")
            K, Q, _, _ = A.sections(c, o["qkv"], o["dout"])
            assert np.array_equal(K, np.round(K)) and np.array_equal(Q, np.round(Q)) and np.abs(K).max() <= A.BIG_C
            if c.dh == 32:
                assert A.padded_boundary_margin(c, o["qkv"], o["dout"]) > 0.5, c.id
        r = A.references(c.id, BF, "big")
        pad = ~c.valid()
        spans.append(float((r["lse0"].transpose(0, 2, 1)[pad] + 1e9).max()))
        assert spans[-1] >= 64.0, f"{c.id}: no padded row's maximum left -1e9"
    assert max(spans) >= 192.0  # several multiples of 64


# ------------------------------------------------------------------------------------------ the table against the launch decision
def test_abi_exports_the_form_queries(ops):
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    assert lib.mst_version() >= 107
    assert len(_lib.SIGNATURES["mst_attn_fwd_form"][1]) == 15 and len(_lib.SIGNATURES["mst_attn_bwd_form"][1]) == 13


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.id)
def test_every_case_gets_the_form_it_is_meant_for(ops, monkeypatch, c):
    for dtype in A.DTYPES:
        f, b = _forms(ops, c, monkeypatch, dtype)
        assert not A.check_forms(c, f, b), "the launch takes another plan than the case is meant for"
        assert f == A.fwd_form(c.B, c.S, c.H, c.dh, c.q_limit, c.fused, c.force), "the restated decision differs from the library's"
        assert b == A.bwd_form(c.B, c.S, c.H, c.dh, c.q_limit, c.force)
    assert f["lds"] <= 160 * 1024 - 1024 and b["lds"] <= 160 * 1024 - 1024


def _fkey(dh, f):
    return (dh, f["path"], f["lone"])


def _bkey(dh, b):
    return (dh, b["path"], b["sparse"], b["lone"], b["dq_chunks"])


def test_the_table_reaches_every_form_the_decision_can_return(ops, monkeypatch):
    """every (head size, path, lone row) forward and (head size, path, sparse, lone row, dQ chunks) backward that some admissible
    shape gets, by the library's decision over S = 1..1500, has a case; the restatement agrees with the library on the whole sweep;
    and the two forms the host code names but no shape reaches stay unreached"""
    reach_f, reach_b = set(), set()
    for force in (None, "stream"):
        if force:
            monkeypatch.setenv("MST_ATTN_PATH", force)
        else:
            monkeypatch.delenv("MST_ATTN_PATH", raising=False)
        for dh in (16, 32, 64):
            H, B = 2, 1
            D = H * dh
            for S in range(1, 1501):
                for ql in (0, 1, 40):
                    for fused in (False, True):
                        f = ops.attn_fwd_form(BF, B, S, H, dh, 0, D, 2 * D, 3 * D, D, ql, fused, D, D)
                        assert f == A.fwd_form(B, S, H, dh, ql, fused, force), (force, dh, S, ql, fused)
                        reach_f.add(_fkey(dh, f))
                    b = ops.attn_bwd_form(BF, B, S, H, dh, 0, D, 2 * D, 3 * D, D, 3 * D, ql)
                    assert b == A.bwd_form(B, S, H, dh, ql, force), (force, dh, S, ql)
                    reach_b.add(_bkey(dh, b))
    have_f, have_b = set(), set()
    for c in A.CASES:
        f, b = _forms(ops, c, monkeypatch)
        have_f.add(_fkey(c.dh, f))
        have_b.add(_bkey(c.dh, b))
    assert not reach_f - have_f, f"forward forms without a case: {sorted(reach_f - have_f)}"
    assert not reach_b - have_b, f"backward forms without a case: {sorted(reach_b - have_b)}"
    assert {p for _, p, _ in reach_f} == set(A.FWD_PATHS) and {p for _, p, *_ in reach_b} == set(A.BWD_PATHS)
    assert not any(k[4] == 4 for k in reach_b), "dQ in 4 chunks became reachable: give it a case"
    assert (64, "chunked", 0) not in reach_f and (16, "chunked", 0) not in reach_f, "a chunked forward beyond head size 32: give it a case"


@pytest.mark.parametrize("dh, S, fwd, bwd", [
    (32, 608, "resident-3", "resident"), (32, 609, "resident-2", "resident"), (32, 864, "resident-2", "resident"),
    (32, 865, "chunked", "stream+chunked-dq"), (32, 896, "chunked", "stream+chunked-dq"), (32, 897, "stream", "stream"),
    (32, 928, "stream", "stream"), (32, 929, "chunked", "stream+chunked-dq"), (32, 1024, "chunked", "stream+chunked-dq"),
    (32, 1025, "stream", "stream"),
    (16, 960, "resident-3", "resident"), (16, 961, "resident-2", "resident"), (16, 1312, "resident-2", "resident"),
    (16, 1313, "resident-2", "stream"), (16, 1376, "resident-2", "stream"), (16, 1377, "stream", "stream"),
    (64, 352, "resident-3", "resident"), (64, 353, "resident-2", "resident"), (64, 512, "resident-2", "resident"),
    (64, 513, "stream", "stream")])
def test_dispatch_edges(ops, monkeypatch, dh, S, fwd, bwd):
    """the sequence lengths at which a launch changes its path, pinned: a change of the LDS budget, of a tile's stride or of a
    condition in attn_fwd_form / attn_bwd_form moves one of them"""
    monkeypatch.delenv("MST_ATTN_PATH", raising=False)
    D = 2 * dh
    assert ops.attn_fwd_form(BF, 1, S, 2, dh, 0, D, 2 * D, 3 * D, D)["path"] == fwd
    assert ops.attn_bwd_form(BF, 1, S, 2, dh, 0, D, 2 * D, 3 * D, D, 3 * D)["path"] == bwd


def test_dispatch_edges_of_the_fused_call_the_lone_row_q_limit_and_the_grid(ops, monkeypatch):
    monkeypatch.delenv("MST_ATTN_PATH", raising=False)
    f = lambda S, H=2, dh=32, ql=0, fused=True, B=1: ops.attn_fwd_form(BF, B, S, H, dh, 0, H * dh, 2 * H * dh, 3 * H * dh, H * dh, ql, fused, H * dh, H * dh)  # noqa: E731
    b = lambda S, H=2, dh=32, ql=0, B=1: ops.attn_bwd_form(BF, B, S, H, dh, 0, H * dh, 2 * H * dh, 3 * H * dh, H * dh, 3 * H * dh, ql)  # noqa: E731
    assert [f(S)["path"] for S in (160, 161, 512, 513)] == ["resident-3", "fused", "fused", "resident-3"]
    assert f(200, fused=False)["path"] == "resident-3" and f(200, H=1)["path"] == "resident-3"   # (D = 32: not a whole 64-deep slice)
    assert f(200, dh=16)["path"] == "resident-3" and f(200, dh=64)["path"] == "resident-3"
    assert f(161)["waves"] == 6 and f(512)["waves"] == 16 and f(544, fused=False)["waves"] == 16 and b(288, dh=64)["waves"] == 8
    # the lone row: head size 16, S = 32 n + 1 > 32, every query produced forward, dense backward
    assert [f(S, dh=16, fused=False)["lone"] for S in (1, 33, 34, 65, 257, 1025)] == [0, 1, 0, 1, 1, 1]
    assert f(257, dh=16, ql=256, fused=False)["lone"] == 0 and f(257, dh=16, ql=257, fused=False)["lone"] == 1 and f(257, fused=False)["lone"] == 0
    assert [b(257, dh=16, ql=ql)["lone"] for ql in (0, 1, 32, 33, 257)] == [1, 0, 0, 1, 1]
    # q_limit: sparse backward for 1..32 below S, dense otherwise; the streaming output grid covers the produced queries alone
    assert [b(100, ql=ql)["sparse"] for ql in (-1, 0, 1, 2, 31, 32, 33, 99, 100, 105)] == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
    assert [b(20, ql=ql)["sparse"] for ql in (19, 20, 32)] == [1, 0, 0]
    assert [(f(928, ql=ql)["grid_stats"], f(928, ql=ql)["grid_out"]) for ql in (0, 1, 128, 129, 927, 928, 933)] == \
        [(8, 8), (8, 1), (8, 1), (8, 2), (8, 8), (8, 8), (8, 8)]
    # the grid: more than 1024 workgroups share a CU, fewer waves each
    assert (f(170, H=32, dh=16, B=33, fused=False)["waves"], b(170, H=32, dh=16, B=33)["waves"]) == (6, 3)
    assert (f(170, H=2, dh=16, fused=False)["waves"], b(170, H=2, dh=16)["waves"]) == (6, 6)
    # forced streaming: dQ in one chunk up to 26 blocks
    monkeypatch.setenv("MST_ATTN_PATH", "stream")
    assert [b(S)["dq_chunks"] for S in (1, 70, 832, 833, 865)] == [1, 1, 1, 0, 2] and f(200)["path"] == "stream"
    assert b(70, dh=64)["path"] == "stream" and b(70, dh=16)["path"] == "stream"


def test_rejected_arguments(ops):
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    form = (ctypes.c_int64 * 8)()
    fwd = lambda **kw: lib.mst_attn_fwd_form(*[{**dict(dtype=0, B=2, S=64, H=2, dh=32, ld=192, k=0, q=64, v=128, ldo=64, ql=0, fused=0, ldx=64,  # noqa: E731
                                                       ldw=64), **kw}[k] for k in ("dtype", "B", "S", "H", "dh", "ld", "k", "q", "v", "ldo", "ql", "fused", "ldx", "ldw")], form)
    bwd = lambda **kw: lib.mst_attn_bwd_form(*[{**dict(dtype=0, B=2, S=64, H=2, dh=32, ld=192, k=0, q=64, v=128, lddo=64, lddq=192, ql=0),  # noqa: E731
                                                **kw}[k] for k in ("dtype", "B", "S", "H", "dh", "ld", "k", "q", "v", "lddo", "lddq", "ql")], form)
    assert fwd() == 0 and bwd() == 0 and fwd(fused=1) == 0
    for call in (fwd, bwd):
        for kw, text in ((dict(S=0), b"must be positive"), (dict(dh=48), b"head size must be 16, 32 or 64"), (dict(ld=196), b"multiples of 8"),
                         (dict(q=60), b"multiples of 8"), (dict(B=32768, H=2), b"too large for grid.y")):
            assert call(**kw) == -1 and text in lib.mst_last_error(), kw
        assert call(dtype=2) == -3 and b"unsupported activation dtype" in lib.mst_last_error()
    assert fwd(ldo=56) == -1 and b"ld_out < H*dh" in lib.mst_last_error()
    assert bwd(lddo=56) == -1 and bwd(lddo=68) == -1 and bwd(lddq=196) == -1 and b"bad leading dims" in lib.mst_last_error()
    for kw in (dict(ldx=56), dict(ldw=68), dict(ld=184), dict(ldo=56)):
        assert fwd(fused=1, **kw) == -1 and b"cover the model width" in lib.mst_last_error(), kw
    assert fwd(fused=1, v=136) == -1 and b"beyond the 3 D weight rows" in lib.mst_last_error()
    assert fwd(ldx=0, ldw=0) == 0  # (the plain call does not look at them)
    assert lib.mst_attn_fwd_form(0, 2, 64, 2, 32, 192, 0, 64, 128, 64, 0, 0, 0, 0, None) == -1 and b"null form" in lib.mst_last_error()
    assert lib.mst_attn_bwd_form(0, 2, 64, 2, 32, 192, 0, 64, 128, 64, 192, 0, None) == -1
    # the launches refuse the same arguments with the same words, before any HIP call
    assert lib.mst_attn_keysoftmax_fwd(0, 2, 64, 2, 48, None, 192, 0, 64, 128, None, None, None, 64, 0, None) == -1
    assert b"head size must be 16, 32 or 64" in lib.mst_last_error()
    assert lib.mst_attn_keysoftmax_bwd(0, 2, 64, 2, 32, None, 196, 0, 64, 128, None, None, None, 64, None, 192, None, 0, None) == -1
    assert b"multiples of 8" in lib.mst_last_error()


def test_the_launches_check_in_a_fixed_order_and_say_which_check_failed():
    """Every launching entry point, called with nothing but null pointers (each check returns before any HIP call): the code and the
    whole text of a bad head size, of a null pointer, and of a bad leading dimension together with a null pointer. The shape is
    looked at first; then the pointers, then the leading dimensions — but for mst_attn_qkv_fwd, whose leading dimensions come first."""
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    N = None
    # (dh, ld of the first operand that has one beside ld_qkv) -> the call
    calls = {
        "mst_attn_keysoftmax_fwd": lambda dh, ld: lib.mst_attn_keysoftmax_fwd(0, 2, 64, 2, dh, N, 192, 0, 64, 128, N, N, N, ld, 0, N),
        "mst_attn_qkv_fwd": lambda dh, ld: lib.mst_attn_qkv_fwd(0, 2, 64, 2, dh, N, ld, N, 64, N, N, 192, 0, 64, 128, N, N, N, 64, 0, N),
        "mst_attn_keysoftmax_bwd": lambda dh, ld: lib.mst_attn_keysoftmax_bwd(0, 2, 64, 2, dh, N, 192, 0, 64, 128, N, N, N, ld, N, 192, N, 0, N),
        "mst_attn_proj_bwd": lambda dh, ld: lib.mst_attn_proj_bwd(0, 2, 64, 2, dh, N, 192, 0, 64, 128, N, N, N, ld, N, 64, N, 64, N, 192, N, N),
    }
    for name, call in calls.items():
        null = name.encode() + b": null pointer"
        both = b"mst_attn_qkv_fwd: leading dimensions must be multiples of 8 and cover the model width" if name == "mst_attn_qkv_fwd" else null
        for (dh, ld), text in (((48, 64), b"attention: head size must be 16, 32 or 64 (got 48)"), ((32, 64), null), ((32, 56), both)):
            assert call(dh, ld) == -1 and lib.mst_last_error() == text, (name, dh, ld, lib.mst_last_error())


# ------------------------------------------------------------------------------------------ the bound
SMALLEST = ("d32-res3-s100-qlS+5", "d64-res2-s353", "d32-chunk-s865", "d32-fused-s161", "d32-forced-s70", "d64-forced-b3-s100")
"""the smallest ragged case of every forward path (three tiles, two tiles, chunked, fused, streaming), which between them take every
backward path too (resident; streaming with dQ in 2 chunks, in 1 chunk, streaming dQ)"""


def _reference(cid, dtype, mode):
    c = A.CASE[cid]
    if not c.fused:
        return c, A.operands(cid, dtype, mode), A.references(cid, dtype, mode)
    o = A.operands(cid, dtype, mode)
    ref, _ = A.qkv_ref(c, o, dtype)
    ldq = c.lds[0]
    qkv = torch.full((c.B * c.S, ldq), float("nan"), dtype=dtype)
    qkv[:, :3 * c.D] = torch.from_numpy(ref).float().to(dtype)   # (row c of W is output column c, wherever the sections sit)
    o = dict(o, qkv=qkv)
    return c, o, A.reference_on(c, qkv, o["dout"], dtype, mode)


def _outside(r, got, c):
    """names of the results with an element outside the bound"""
    bad = []
    for k in A.RESULTS:
        b = r["b_" + k]
        if not (np.abs(got[k] - r[k]) <= b).all():
            bad.append(k)
    return bad


def _with_lse(r):
    return dict(r, lse=r["lse0"] + r["lse1"])


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("dtype", A.DTYPES, ids=lambda d: A.DT_NAME[d])
@pytest.mark.parametrize("cid", SMALLEST)
def test_the_bound_accepts_a_cpu_emulation_that_rounds_where_the_kernels_round(cid, dtype, mode):
    """fp32 logits, P and g rounded to the activation type before they are summed, delta from the unrounded dV, results rounded"""
    c, o, r = _reference(cid, dtype, mode)
    K, Q, V, dO = A.sections(c, o["qkv"], o["dout"])
    emu = _with_lse(A.attn_ref(K, Q, V, c.valid(mode), dO, c.q_limit, emulate=dtype))
    assert not _outside(r, emu, c)
    worst = {k: float(np.max(np.abs(emu[k] - r[k]) / np.maximum(r["b_" + k], 1e-300))) for k in ("out", "dV", "dK", "dQ")}
    print(f"\n{cid} {A.DT_NAME[dtype]} {mode}: emulation error / bound {worst}")
    if mode == "big":
        assert max(worst.values()) > 0.05, "the bound is too slack to tell a rounding from a missing term"


@pytest.mark.parametrize("mode", A.MODES)
def test_the_exponentials_argument_error_measured_in_fp32_is_inside_rho(mode):
    """the fast form's fp32 steps emulated (sk2, ck2, one fma, exp2 in float32; statistics rounded to fp32) against the fp64
    probabilities, on the unpadded keys of a small case: worst error / rho measured 0.022 (real) and 0.010 (big); asserted below
    1 / 2, the factor the constants of attn_refs carry"""
    c = A.CASE["d32-res3-s64"]
    o, r = A.operands(c.id, BF, mode), A.references(c.id, BF, mode)
    K, Q, _, _ = A.sections(c, o["qkv"], o["dout"])
    valid, f32 = c.valid(mode), np.float32
    worst = 0.0
    for b in range(c.B):
        if not valid[b].any():
            continue
        x = (K[b, :, 0] @ Q[b, :, 0].T).astype(f32)
        m, logl = r["lse0"][b, 0].astype(f32), r["lse1"][b, 0].astype(f32)
        log2e = f32(1.4426950408889634)
        sk2 = f32(f32(A.scale_of(c.dh)) * log2e)
        ck2 = (-(m + logl)).astype(f32) * log2e
        arg = (x.astype(np.float64) * float(sk2) + ck2.astype(np.float64)[:, None]).astype(f32)   # one rounding: the fma
        with np.errstate(over="ignore"):   # (padded keys: not this form's, masked out below)
            p = np.exp2(arg).astype(np.float64)
        t = A.logits32(K[b, :, 0] @ Q[b, :, 0].T, A.scale_of(c.dh), valid[b])
        P = np.exp(t - (r["lse0"][b, 0] + r["lse1"][b, 0])[:, None])
        keep = valid[b][:, None] & (P > 1e-30)
        worst = max(worst, float((np.abs(p - P) / P / r["rho"][b, 0])[keep].max()))
    print(f"\n{mode}: fp32 argument emulation, worst relative error of P / rho = {worst:.3f}")
    assert worst < 0.5


def _mutation_cases():
    for cid in SMALLEST:
        c = A.CASE[cid]
        for mut in A.MUTATIONS:
            dtype, mode = BF, "real"
            if mut == "padded_uniform":
                mode = "big"      # (in real mode a padded row IS uniform)
                if c.fused:
                    continue      # (a fused call has no padded key in big mode: attn_refs.operands)
            if mut == "p_rounded_bf16":
                dtype, mode = FP, "big"   # few-hot rows: one rounding is not averaged away among hundreds
            yield pytest.param(cid, mut, dtype, mode, id=f"{cid}-{mut}")


@pytest.mark.parametrize("cid, mut, dtype, mode", list(_mutation_cases()))
def test_the_bound_refuses_a_wrong_result(cid, mut, dtype, mode):
    c, o, r = _reference(cid, dtype, mode)
    K, Q, V, dO = A.sections(c, o["qkv"], o["dout"])
    wrong = _with_lse(A.attn_ref(K, Q, V, c.valid(mode), dO, c.q_limit, mut=mut))
    bad = _outside(r, wrong, c)
    assert bad, f"{cid} {mode}: {mut} stays inside the bound of every result"
    for dt in A.DTYPES:   # ... in either type where the mutation does not depend on it
        if mut != "p_rounded_bf16" and dt != dtype:
            c2, o2, r2 = _reference(cid, dt, mode)
            K, Q, V, dO = A.sections(c2, o2["qkv"], o2["dout"])
            assert _outside(r2, _with_lse(A.attn_ref(K, Q, V, c2.valid(mode), dO, c2.q_limit, mut=mut)), c2), f"{cid} {A.DT_NAME[dt]}: {mut}"
