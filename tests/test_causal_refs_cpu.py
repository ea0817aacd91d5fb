"""tests/causal_refs.py without a GPU: the fp64 reference against torch autograd in fp64 and against an answer worked out by hand,
the completeness of the case table, what the `late` and `early` operands are built to force, the derived tolerance — it accepts an
emulation that rounds where the kernels round and refuses every wrong result listed in causal_refs.MUTATIONS — and the arguments
mst_attn_causal_fwd / _bwd reject beyond those of tests/test_causal_cpu.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import causal_refs as C  # noqa: E402

BF, FP = C.BF, C.FP


# ------------------------------------------------------------------------------------------ the reference itself
def _torch_causal(c, o):
    """fp64 autograd on the flat qkv layout (its own indexing, not causal_refs.sections), masked as tests/test_causal_cpu.py's
    causal_attention masks, without the projections. A row without keys is NaN there; here it gets constant logits and its
    probabilities are multiplied by 0, which is the contract: no output and no gradient."""
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    qkv = torch.nan_to_num(o["qkv"].double(), nan=0.0).requires_grad_(True)
    x3 = qkv.view(B, S, -1)
    heads = lambda off: x3[:, :, off:off + D].reshape(B, S, H, dh).transpose(1, 2)  # noqa: E731   [B, H, S, dh]
    K, Q, V = (heads(off) for off in c.offs)
    logits = torch.matmul(Q, K.transpose(-1, -2)) * C.scale_of(dh)
    allowed = torch.ones(S, S, dtype=torch.bool).tril()[None, None] & (o["keymask"] > 0)[:, None, None, :]
    has = allowed.any(-1, keepdim=True)
    masked = torch.where(has, logits.masked_fill(~allowed, float("-inf")), torch.zeros_like(logits))
    probs = torch.softmax(masked, dim=-1) * has
    out = torch.matmul(probs, V)                                                      # [B, H, S, dh]
    dO = torch.nan_to_num(o["dout"].double(), nan=0.0)[:, :D].view(B, S, H, dh).transpose(1, 2)
    (out * dO).sum().backward()
    g = qkv.grad.view(B, S, -1)
    dK, dQ, dV = (g[:, :, off:off + D].reshape(B, S, H, dh).numpy() for off in c.offs)
    lse = torch.where(has[..., 0], torch.logsumexp(masked, dim=-1), torch.full_like(masked[..., 0], float("-inf")))
    delta = (dO * out).sum(-1)                                                       # rowsum(dO o O) = sum_k P dP
    return dict(out=out.detach().transpose(1, 2).numpy(), lse=lse.detach().numpy(), delta=delta.detach().numpy(), dQ=dQ, dK=dK, dV=dV), \
        has[..., 0].expand(B, H, S).numpy()


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("cid", ["d16-s1-b3h2-plain", "d32-s31-b2h1-perm", "d64-s32-b3h8-wide", "d16-s33-b2h2-wide", "d32-s64-b2h1-wide",
                                 "d64-s65-b3h8-wide", "d16-s97-b2h8-plain", "d32-s257-b2h2-perm"])
def test_reference_equals_torch_autograd_in_fp64(cid, mode):
    """full, prefix, hole, masked key 0 and masked block, rows without keys, all three layouts, all three operand modes"""
    c = C.CASE[cid]
    o, r = C.operands(cid, BF, mode), C.references(cid, BF, mode)
    want, has = _torch_causal(c, o)
    for k in C.RESULTS:
        got, ref = r[k], want[k]
        if k == "lse":
            assert np.array_equal(np.isfinite(got), has) and (got[~has] == -np.inf).all() and (ref[~has] == -np.inf).all()
            got, ref = got[has], ref[has]
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        err = np.abs(got - ref).max() if got.size else 0.0
        assert err <= 1e-9 * max(1.0, np.abs(ref).max()), f"{cid} {mode}: {k} off by {err}"
    if not has.all():   # the contract of the rows without keys, spelled out
        e = ~has                                                   # [B, H, S]
        assert (r["lse0"][e] == -np.inf).all() and (r["lse1"][e] == -np.inf).all() and not r["delta"][e].any()
        assert not r["out"].transpose(0, 2, 1, 3)[e].any() and not r["dQ"].transpose(0, 2, 1, 3)[e].any()


def test_zero_queries_give_the_mean_of_the_admissible_values_as_worked_out_by_hand():
    """Q = 0: every logit is 0, every row uniform over its n admissible keys: out = their mean of V, lse0 = 0, lse1 = log n, dV[k] =
    sum over the queries that admit k of dO[q] / n[q]; key 0 and a hole are masked, so query 0 has no key at all"""
    rng = np.random.default_rng(11)
    S, dh = 41, 16
    K, V, dO = (rng.standard_normal((S, dh)) for _ in range(3))
    valid = np.ones(S, dtype=bool)
    valid[0] = valid[17:23] = False
    r = C.head_ref(np.zeros((S, dh)), K, V, valid, dO, dh)
    dV = np.zeros((S, dh))
    for q in range(S):
        keys = [k for k in range(q + 1) if valid[k]]
        n = len(keys)
        if not n:
            assert q == 0 and not r["out"][q].any() and r["lse0"][q] == -np.inf and r["lse1"][q] == -np.inf and r["delta"][q] == 0.0
            continue
        assert np.allclose(r["out"][q], V[keys].mean(0), rtol=0, atol=1e-13)
        assert r["lse0"][q] == 0.0 and abs(r["lse1"][q] - math.log(n)) < 1e-13
        assert abs(r["delta"][q] - dO[q] @ V[keys].mean(0)) < 1e-12
        dV[keys] += dO[q] / n
    assert np.allclose(r["dV"], dV, rtol=0, atol=1e-12) and not r["dV"][~valid].any() and not r["dK"][~valid].any()
    assert np.allclose(r["dK"], 0.0, atol=1e-13)   # (dK = scale sum_q dS Q with Q = 0)


# ------------------------------------------------------------------------------------------ the table
def test_the_table_is_complete():
    assert len({c.id for c in C.CASES}) == len(C.CASES)
    assert {c.S for c in C.CASES} == {1, 31, 32, 33, 64, 65, 97, 257} and {c.H for c in C.CASES} == {1, 2, 8}
    assert all(c.B * c.H <= 24 for c in C.CASES)
    big = max(C.CASES, key=lambda c: c.B * c.H * c.S * c.S)
    assert (big.B, big.H, big.S) == (2, 2, 257)
    for dh in (16, 32, 64):   # every case runs in both types, so a head size that meets something meets it in bf16 and in fp16
        mine = [c for c in C.CASES if c.dh == dh]
        assert {c.S for c in mine} == {1, 31, 32, 33, 64, 65, 97, 257}
        assert {c.s_class for c in mine} == set(C.S_CLASSES)
        assert {m for c in mine for m in c.masks} == set(C.MASK_KINDS)
        assert any(len(set(c.masks[:c.B])) > 1 for c in mine), "no batch whose rows differ"
        assert {c.layout for c in mine} == {"plain", "wide", "perm"}
    for c in C.CASES:
        D = c.D
        if c.layout == "wide":
            assert c.lds == (3 * D + 8, D + 8, D + 16) and c.offs == (0, D, 2 * D)
        if c.layout == "perm":
            assert c.offs == (2 * D, 0, D) and c.lds == (3 * D, D, D)      # k_off, q_off, v_off
        v = c.valid()
        if "key0" in c.masks[:c.B]:
            assert (~v[:, 0]).any()
        if "block" in c.masks[:c.B]:
            assert any((~v[b, 32 * kb:32 * (kb + 1)]).all() for b in range(c.B) for kb in range(c.NB))
        if "hole" in c.masks[:c.B]:   # masked keys with admissible ones on both sides
            b = c.masks.index("hole")
            mid = c.S // 2
            assert v[b, :mid].any() and not v[b, mid:mid + 9].any() and v[b, mid + 9:].any()


def _rows(c, o):
    """per (batch, head): the logits with the excluded pairs at -inf"""
    Q, K, _, _ = C.sections(c, o["qkv"], o["dout"])
    S = c.S
    tril = np.tril(np.ones((S, S), dtype=bool))
    for b in range(c.B):
        adm = tril & c.valid()[b][None, :]
        for h in range(c.H):
            yield np.where(adm, Q[b, :, h] @ K[b, :, h].T * C.scale_of(c.dh), -np.inf), adm


@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: C.DT_NAME[d])
@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c.id)
def test_operands_stay_finite_and_the_late_and_early_modes_force_what_they_are_built_for(c, dtype):
    blk = np.arange(c.S) // 32
    seen_rescale = seen_underflow = False
    for mode in C.MODES:
        o, r = C.operands(c.id, dtype, mode), C.references(c.id, dtype, mode)
        for a in C.sections(c, o["qkv"], o["dout"]):
            assert np.isfinite(a).all() and np.abs(a).max() < 65504.0
        for k, a in r.items():
            assert not np.isnan(a).any() and (np.isfinite(a).all() or k in ("lse", "lse0", "lse1")), f"{mode}: {k}"
        if mode == "real":
            continue
        for t, adm in _rows(c, o):
            for q in range(c.S):
                blocks = np.unique(blk[adm[q]])
                if not len(blocks):
                    continue
                mx = np.array([t[q, (blk == kb) & adm[q]].max() for kb in blocks])
                if mode == "late":    # the running maximum grows in every admissible block, by more than 20 ln 2: alpha < 2^-20
                    assert (np.diff(mx) > 20.0 * math.log(2.0)).all(), f"row {q}: block maxima {mx}"
                    seen_rescale |= len(blocks) > 1
                else:                 # the maximum sits in the first admissible block; every later e is 0 in the activation type
                    later = adm[q] & (blk > blocks[0])
                    assert mx.argmax() == 0 and not C.round_to(np.exp(t[q, later] - mx[0]), dtype).any(), f"row {q}"
                    seen_underflow |= bool(later.any())
    if c.NB > 1:
        assert seen_rescale and seen_underflow


# ------------------------------------------------------------------------------------------ the bound
def _outside(r, got):
    """names of the results with an element outside the bound"""
    return [k for k in C.RESULTS if C.violations(r, got, k).any()]


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: C.DT_NAME[d])
@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c.id)
def test_the_bound_accepts_a_cpu_emulation_that_rounds_where_the_kernels_round(c, dtype, mode):
    """fp32 logits and dP, e, P and dS rounded to the activation type before they are summed, fp32 statistics, results rounded"""
    r = C.references(c.id, dtype, mode)
    emu = C.variant(c.id, dtype, mode, emulate=dtype)
    assert not _outside(r, emu)
    worst = {k: float(C.ratios(r, emu, k).max()) for k in C.RESULTS}
    print(f"\n{c.id} {C.DT_NAME[dtype]} {mode}: emulation error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
    if c.S == 1:
        # one key: P = 1, so out = V, dV = dO and dS = 0 whatever is rounded — no 16-bit rounding for a floor to be held against
        assert all(np.array_equal(emu[k], r[k]) for k in ("out", "dV")) and not emu["dQ"].any() and not emu["dK"].any()
    else:
        assert max(worst.values()) > 0.05, "the bound is too slack to tell a rounding from a missing term"


def _suited(mut, c):
    masked = {m for m in c.masks[:c.B]} - {"full"}
    return {"drop_block": c.NB >= 2, "stale_rescale": c.NB >= 2, "rows_beyond_s_counted": c.S % 32 != 0 and c.S > 1,
            "empty_row_nan": bool((~c.valid()[:, 0]).any()), "mask_ignored_in_backward": bool(masked) and c.S > 1,
            "block_granular_causality": c.S > 1, "delta_shifted": c.S > 1, "kq_swapped": c.S > 1, "softmax_over_queries": c.S > 1,
            "row_group_swapped": c.S > 4, "p_rounded_bf16": c.S > 1, "wrong_scale": c.S > 1}.get(mut, True)


def _mutation_cases():
    for mut in C.MUTATIONS:
        for c in C.CASES:
            if c.S <= 97 and _suited(mut, c):
                yield pytest.param(mut, c, id=f"{mut}-{c.id}")


def test_every_mutation_has_suited_cases_at_every_head_size():
    got = {(p.values[0], p.values[1].dh) for p in _mutation_cases()}
    assert got == {(m, dh) for m in C.MUTATIONS for dh in (16, 32, 64)}


@pytest.mark.parametrize("mut, c", list(_mutation_cases()))
def test_the_bound_refuses_a_wrong_result(mut, c):
    """in every case that can show the mutation, in both types, some result has an element outside its bound: on unit-scale
    operands, and where the mutation is about the rescale or the rounding of P on the operands built for it"""
    # (stale_rescale on unit-scale operands too from S = 64 on: at S = 33 the one row of the last block may have no key there that
    # raises its maximum, and then there is nothing stale)
    modes = {"stale_rescale": ("late", "real") if c.S >= 64 else ("late",), "p_rounded_bf16": ("real", "early")}.get(mut, ("real",))
    for mode in modes:
        for dtype in ((FP,) if mut == "p_rounded_bf16" else C.DTYPES):
            r = C.references(c.id, dtype, mode)
            bad = _outside(r, C.variant(c.id, dtype, mode, mut=mut))
            assert bad, f"{c.id} {C.DT_NAME[dtype]} {mode}: {mut} stays inside the bound of every result"


# ------------------------------------------------------------------------------------------ the entry points' argument checks
def test_causal_entry_points_reject_bad_leading_dimensions_alignment_and_grids():
    """each call differs in ONE argument from a set the checks accept; nothing is launched (validation comes first)"""
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    arr = np.zeros(4096, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16   # (never dereferenced)
    f = dict(dtype=0, B=2, S=8, H=2, dh=16, qkv=buf, ld=96, k=0, q=32, v=64, km=buf, lse=buf, out=buf, ldo=32, stream=None)
    b = dict(dtype=1, B=2, S=8, H=2, dh=16, qkv=buf, ld=96, k=0, q=32, v=64, km=buf, lse=buf, dout=buf, lddo=32, dqkv=buf, lddq=96,
             delta=buf, stream=None)

    def refused(name, base, text, **kw):
        with pytest.raises(_lib.MstError):
            _lib.call(name, *{**base, **kw}.values())
        assert text in lib.mst_last_error(), (kw, lib.mst_last_error())

    for kw in (dict(ldo=24), dict(ldo=36), dict(out=buf + 8)):
        refused("mst_attn_causal_fwd", f, b"out must be 16-byte aligned with ld_out a multiple of 8 and >= H*dh", **kw)
    for kw in (dict(lddo=24), dict(lddo=36), dict(dout=buf + 8)):
        refused("mst_attn_causal_bwd", b, b"dout must be 16-byte aligned with ld_dout a multiple of 8 and >= H*dh", **kw)
    for kw in (dict(lddq=88), dict(lddq=100), dict(dqkv=buf + 8), dict(lddq=56)):
        refused("mst_attn_causal_bwd", b, b"dqkv must be 16-byte aligned with ld_dqkv a multiple of 8 that covers every section", **kw)
    for name, base in (("mst_attn_causal_fwd", f), ("mst_attn_causal_bwd", b)):
        refused(name, base, b"too large for grid.y", B=32768)          # B H = 65536
        refused(name, base, b"a section runs past ld_qkv", ld=88)
        refused(name, base, b"16-byte aligned pointer", qkv=buf + 8)
