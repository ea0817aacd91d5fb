"""The stand-alone row kernels of csrc/embed.hip and mst_segment_sumsq on a real MI355X against the fp64 references of
tests/rowkernel_refs.py: mst_embed_fwd, mst_embed_bwd, mst_group_colsum (its thread map asserted from mst_group_colsum_form),
mst_mask_from_lengths and mst_segment_sumsq, in bf16 and fp16 where a type applies, every element held to its derived bound, every pad
column and guard row left alone, every case run twice (the sums are atomics: both runs are held to the bound, neither to the other),
and every refusal of these entry points leaving every output buffer untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowkernel_refs as K  # noqa: E402

pytestmark = pytest.mark.gpu


def _report(cid, results):
    print(f"\n{cid}: worst error / bound " + ", ".join(f"{r.name} {r.ratio:.3f}" for r in results))
    for r in results:
        assert not r.bad.any(), (f"{cid}: {r.name} ({r.stage}): {int(r.bad.sum())}/{r.bad.size} elements outside the bound, worst {r.ratio:.3g} bounds, "
                                 f"first at {tuple(np.argwhere(np.atleast_1d(r.bad))[0])}")


def _view3(c, t, S):
    """[B * S + guard, ld] -> the [B, S, D] view the wrappers take (row stride ld)"""
    return t[:c.B * S].view(c.B, S, t.shape[1])[:, :, :c.D]


@pytest.mark.parametrize("c", [c for c in K.EMBED_CASES if c.fwd], ids=lambda c: c.id)
def test_embed_fwd_against_fp64(gpu, c):
    from musicstyletransfer_amd import ops as o
    ins = K.embed_operands(c)
    i = {k: v.to(gpu) for k, v in ins.items()}
    for run in range(2):
        u = {k: v.to(gpu) for k, v in K.embed_fwd_outputs(c).items()}
        o.embed_fwd(i["tokens"], i["table"][:, :c.D], i["pos"][:, :c.D], _view3(c, u["out"], c.S_out), c.s_off, c.alpha,
                    classes=i["classes"] if c.cls else None, cls_table=i["cls_table"][:, :c.D] if c.cls else None,
                    keymask=u.get("keymask"), keep=i.get("keep"))
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in u.items()}
        _report(c.id, K.embed_fwd_check(c, ins, got))
        assert K.embed_fwd_intact(c, got) == []


@pytest.mark.parametrize("c", K.EMBED_CASES, ids=lambda c: c.id)
def test_embed_bwd_against_fp64(gpu, c):
    from musicstyletransfer_amd import ops as o
    ins = K.embed_operands(c)
    i = {k: v.to(gpu) for k, v in ins.items()}
    before = K.embed_bwd_outputs(c)
    if c.dcls:
        q = o.group_colsum_form(c.T, c.D)
        assert (q["cpr"], q["rg"], q["grid"]) == (c.D // 8, 256 // (c.D // 8), (c.T + 63) // 64)
    for run in range(2):
        u = {k: v.to(gpu) for k, v in before.items()}
        o.embed_bwd(i["tokens"], u["dtable"][:K.V, :c.D], _view3(c, i["dX"], c.S_out), c.s_off, c.alpha,
                    classes=i["classes"] if c.dcls else None, dcls=u["dcls"][:K.NCLS, :c.D] if c.dcls else None, keep=i.get("keep"))
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in u.items()}
        _report(c.id, K.embed_bwd_check(c, ins, before, got))
        assert K.embed_bwd_intact(c, got) == []


@pytest.mark.parametrize("c", K.COLSUM_CASES, ids=lambda c: c.id)
def test_group_colsum_against_fp64(gpu, c):
    from musicstyletransfer_amd import ops as o
    q = o.group_colsum_form(c.T, c.D)
    assert (q["cpr"], q["rg"], q["grid"], q["lds"]) == c.form
    ins = K.colsum_operands(c)
    i = {k: v.to(gpu) for k, v in ins.items()}
    before = K.colsum_outputs(c)
    for run in range(2):
        u = {k: v.to(gpu) for k, v in before.items()}
        o.group_colsum(_view3(c, i["X"], c.S_out), c.T, c.D, c.s_off, i["idx"], u["dst"][:K.NCLS, :c.D], c.alpha)
        torch.cuda.synchronize()
        got = {k: v.cpu() for k, v in u.items()}
        _report(c.id, K.colsum_check(c, ins, before, got))
        assert K.intact2d("dst", got["dst"], np.arange(K.NCLS), c.D) == []


@pytest.mark.parametrize("c", K.MASK_CASES, ids=lambda c: c.id)
def test_mask_from_lengths_is_exact(gpu, c):
    from musicstyletransfer_amd import ops as o
    lens = torch.from_numpy(c.lens).to(gpu)
    for run in range(2):
        km = torch.full((c.B * c.S + 64,), K.MASK_SENTINEL, dtype=torch.uint8, device=gpu)
        o.mask_from_lengths(lens, c.add, km[:c.B * c.S].view(c.B, c.S))
        torch.cuda.synchronize()
        got = km.cpu().numpy()
        assert (got[:c.B * c.S].reshape(c.B, c.S) == K.mask_ref(c)).all(), c.id
        assert (got[c.B * c.S:] == K.MASK_SENTINEL).all(), "written behind B * S"


@pytest.mark.parametrize("c", K.SEG_CASES, ids=lambda c: c.id)
def test_segment_sumsq_against_fp64(gpu, c):
    from musicstyletransfer_amd import ops as o
    ins = K.seg_operands(c)
    x, ranges = ins["x"].to(gpu), ins["ranges"].to(gpu)
    for run in range(2):
        out = torch.full((c.n + K.GUARD,), K.SENTINEL, dtype=torch.float32, device=gpu)
        o.segment_sumsq(x, ranges, out)
        torch.cuda.synchronize()
        got = out.cpu()
        r, g_inf, w_inf = K.seg_check(ins, got)
        _report(c.id, [r])
        assert (g_inf == w_inf).all(), "a segment that holds an inf sums to inf"
        assert (r.got[r.ref == 0] == 0).all() and (got[c.n:] == K.SENTINEL).all()


def test_every_refusal_leaves_every_output_untouched(gpu):
    """status, message, and after each refused call every buffer a launch could have written still holds its sentinel: the column
    sums' checks of mst_embed_bwd come before its scatter launch"""
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    s = K.REFUSAL_SHAPE
    B, T, D, S = s["B"], s["T"], s["D"], s["S_out"]
    f = lambda *shape, dtype=torch.float32, fill=1.0: torch.full(shape, fill, dtype=dtype, device=gpu)  # noqa: E731
    act = torch.bfloat16
    bufs = dict(tokens=f(B, T, dtype=torch.int32, fill=1), table=f(K.V, D), classes=f(B, dtype=torch.int32, fill=0), cls_table=f(K.NCLS, D),
                pos=f(S, D), keep=f(B * T, dtype=torch.uint8, fill=1), dX=f(B * S, D, dtype=act), lens=f(B, dtype=torch.int32, fill=2),
                x=f(64), ranges=torch.tensor([[0, 4], [4, 8]], dtype=torch.int64, device=gpu))
    outs = dict(out=f(B * S, D, dtype=act, fill=K.SENTINEL), keymask=f(B * S, dtype=torch.uint8, fill=K.MASK_SENTINEL),
                dtable=f(K.V, D, fill=K.SENTINEL), dcls=f(K.NCLS, D, fill=K.SENTINEL))
    bufs["X"], bufs["idx"] = bufs["dX"], bufs["classes"]
    form = (C.c_int64 * 4)()
    ptrs = {k: t.data_ptr() for k, t in {**bufs, **outs}.items()}
    ptrs.update(dst=ptrs["dcls"], form=C.addressof(form))
    # (mst_mask_from_lengths writes keymask, mst_segment_sumsq writes `out`: the same two sentinel buffers serve, both large enough)
    ptrs["stream"] = None
    for entry, changes, status, fragment in K.REFUSALS:
        args = K.refusal_args(entry, changes, ptrs)
        assert getattr(lib, entry)(*args) == status, (entry, changes)
        assert fragment.encode() in lib.mst_last_error(), (entry, changes, lib.mst_last_error())
        torch.cuda.synchronize()
        for name, t in outs.items():
            want = K.MASK_SENTINEL if t.dtype == torch.uint8 else K.SENTINEL
            assert bool((t == want).all()), f"{name} was written by a refused call: {entry} {changes}"
    # ... and the good call the refusals depart from is accepted
    assert lib.mst_embed_bwd(*K.refusal_args("mst_embed_bwd", {}, ptrs)) == 0
    torch.cuda.synchronize()
    assert not bool((outs["dtable"] == K.SENTINEL).all()) and not bool((outs["dcls"] == K.SENTINEL).all())
