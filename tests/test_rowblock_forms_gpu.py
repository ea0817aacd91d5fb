"""The LayerNorm-fused row-block launches on a real MI355X against the fp64 reference of tests/rowblock_refs.py: mst_gemm_nt_ln
(modes 1 and 2), mst_ffn_ln_fwd / mst_proj_ffn_ln_fwd / mst_ffn_ln_bwd / mst_ffn_ln_bwd_lead in all eight kernel forms per width,
the stand-alone mst_layernorm_fwd / _bwd and mst_dec_tail_step, in bf16 and fp16, on operands made to be hard (offset rows, a
constant row, a zero gamma), every stored tensor held stage by stage to its derived bound, every pad column, guard row and row
outside the launch's groups left alone. A failure names the tensor, the stage, the rows and the tiles."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowblock_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(o, c, i, u):
    """the case's launch through the ops wrappers. i: operands on the device, u: output buffers on the device"""
    bufs, _ = R.plan(c)
    _, P = R.rows(c)
    D, F = c.D, c.F

    def v(name):
        """a 2-D buffer without its guard rows and pad columns (the leading dimension stays 8 wider than the width)"""
        b = bufs[name]
        t = u[name] if b.out else i[name]
        if b.rows in ("log", "phys"):
            return t[:(c.M if b.rows == "log" else P), :b.width]
        return t[:, :b.width] if b.rows == "w" else t

    def drop(site, p=c.p):
        return dict(dropout_p=p, dropout_seed=R.SEED, dropout_seed_ptr=i["seed_word"], dropout_site=site) if p > 0 else {}

    def grads(prefix=""):
        return dict(dgamma=u[prefix + "dgamma"], dbeta=u[prefix + "dbeta"], partials=u.get(prefix + "parts"))

    rg = c.groups if c.kind in ("ffn_fwd", "ffn_bwd", "dec_tail") else None
    remap = c.groups if (c.groups is not None and c.kind.startswith("gemm_ln")) else (0, 0, 0)
    if c.kind in ("ffn_fwd", "dec_tail"):
        head = None
        if c.proj or c.kind == "dec_tail":
            head = dict(att=v("att"), W=v("Wp"), h1=v("h1"), gamma=i["g1"], beta=i["be1"], mean=u["mean1"], rstd=u["rstd1"], N=D, K=D,
                        bias=i["bp"], resid=v("xin"), **drop(R.SITE_PROJ))
        ff2 = dict(K=F, bias=i["b2"], **drop(R.SITE_FF2))
        if c.resid == "self":
            ff2["self_resid"] = True
        elif c.resid != "none":
            ff2["resid"] = v("x") if c.resid == "x" else v("r2")
        fwd = dict(x=v("x"), W1=v("W1"), a_out=v("a"), W2=v("W2"), h_out=v("h2"), gamma=i["gamma"], beta=i["beta"], y_out=v("y"),
                   mean=u["mean"], rstd=u["rstd"], ff1=dict(K=D, bias=i["b1"], act=o.ACT_RELU, **drop(R.SITE_FF1)), ff2=ff2, proj=head,
                   row_groups=rg)
        if c.kind == "ffn_fwd":
            o.ffn_ln_fwd(**fwd)
            return
        # the whole last-decoder-layer launch, set up as tests/test_dec_tail_gpu.py does
        dev = u["h2"].device
        Wo = torch.full((128, D + R.PAD), R.NAN, dtype=c.dtype, device=dev)
        Wo[:, :D] = v("Wot").t()
        loss = dict(A=v("y"), B=Wo[:, :D], labels=i["labels"], loss=torch.zeros(c.M // rg[0], device=dev), T=rg[0], dlogits=v("dlogits"),
                    probs=None, label_smoothing=0.1, downweight=True, gscale=1024.0 if c.dtype == R.FP else 4.0, M=c.M, K=D,
                    bias=torch.zeros(128, device=dev), a_remap=rg)
        dgrad = dict(A=v("dlogits"), B=v("Wot"), dX_out=v("dh"), x=v("h2"), gamma=i["gamma"], mean=u["mean"], rstd=u["rstd"], dgamma=None,
                     dbeta=None, mask_mode=2, partials=u["l3_parts"], M=c.M, N=D, K=128, c_remap=rg, **drop(R.SITE_FF2))
        bwd = dict(dff=v("dh"), W2t=v("W2t"), dpre_out=v("dpre"), gate=v("a"), W1t=v("W1t"), dx_out=v("dh1"), x=v("h1"), gamma=i["g1"],
                   mean=u["mean1"], rstd=u["rstd1"], dgamma=None, dbeta=None, alpha=1.0 / (1.0 - c.p), partials=u["parts"], row_groups=rg,
                   dx_masked=v("dh1m"), mask_mode=1, K=F, **drop(R.SITE_PROJ))
        o.dec_tail_step(fwd, loss, dgrad, bwd)
    elif c.kind == "ffn_bwd":
        lead, kw = None, {}
        if c.lead >= 0:
            lead = dict(dy=v("dyl"), x=v("xl"), gamma=i["gl"], mean=i["meanl"], rstd=i["rstdl"], dx=v("dh"),
                        dx_masked=v("dhm") if c.lead == 1 else None, **grads("l_"), **drop(R.SITE_LEAD))
            dff = v("dhm") if c.lead == 1 else v("dh")
            if c.resid == "x":
                kw["resid"] = v("dh")
        else:
            dff = v("dff")
            if c.resid == "other":
                kw["resid"] = v("r")
        if c.mode:
            kw.update(drop(R.SITE_LN))
        o.ffn_ln_bwd(dff, v("W2t"), v("dpre"), v("gate"), v("W1t"), v("dx"), v("x"), i["gamma"], i["mean"], i["rstd"], alpha=c.alpha,
                     dx_masked=v("dxm") if c.mode == 1 else None, mask_mode=c.mode, lead=lead, row_groups=rg, K=F, **grads(), **kw)
    elif c.kind == "gemm_ln_fwd":
        kw = dict(M=c.M, N=D, K=F, alpha=c.alpha, c_remap=remap, self_resid=c.resid == "self", **drop(R.SITE_FF1))
        if c.bias:
            kw["bias"] = i["bias"]
        if c.resid == "other":
            kw["resid"] = v("r")
        o.gemm_nt_ln_fwd(v("A"), v("W"), v("h"), i["gamma"], i["beta"], v("y"), u["mean"], u["rstd"], **kw)
    elif c.kind == "gemm_ln_bwd":
        kw = dict(M=c.M, N=D, K=F, alpha=c.alpha, bias=i["bias"], c_remap=remap)
        if c.resid == "other":
            kw["resid"] = v("r")
        if c.mode:
            kw.update(drop(R.SITE_LN))
        o.gemm_nt_ln_bwd(v("A"), v("W"), v("dx"), v("x"), i["gamma"], i["mean"], i["rstd"], dx_masked=v("dxm") if c.mode == 1 else None,
                         mask_mode=c.mode, **grads(), **kw)
    else:
        stride = c.groups[1]
        o.layernorm_fwd(v("x"), i["gamma"], i["beta"], v("y"), u["mean"], u["rstd"], D=D, M=c.M, row_id_stride=stride)
        o.layernorm_bwd(v("x"), i["gamma"], u["mean"], u["rstd"], v("dy"), v("dx"), D=D, dx_masked=v("dxm") if c.mode == 1 else None,
                        mask_mode=c.mode, M=c.M, row_id_stride=stride, **grads(), **(drop(R.SITE_LN) if c.mode else {}))


def _run(o, c, ins, gpu):
    """one launch into fresh outputs, the partial rows added by mst_partial_sums -> (outputs on the host, the parameter gradients as
    the launch itself left them)"""
    bufs, _ = R.plan(c)
    i = {k: t.to(gpu) for k, t in ins.items()}
    u = {k: t.to(gpu) for k, t in R.outputs(c).items()}
    if c.kind == "ln":  # the instantiation the table claims is the one the library launches, forward and backward
        fwd, bwd = o.layernorm_form(False, c.dtype, c.M, c.D), o.layernorm_form(True, c.dtype, c.M, c.D)
        assert (fwd["nv"], fwd["r"], bwd["r"]) == c.form and bwd["nv"] == fwd["nv"], (c.id, fwd, bwd)
        assert (fwd["waves"], fwd["lds"]) == (4, 0) and bwd["lds"] == 8 * bwd["waves"] * c.D
        assert bwd["grid"] == R.n_parts(c) == o.layernorm_bwd_parts(c.M, c.D)
    elif c.kind != "gemm_ln_fwd" and c.kind != "ffn_fwd":
        assert o.gemm_nt_ln_parts(c.M) == R.n_parts(c)
    _launch(o, c, i, u)
    before, jobs = {}, []
    for name, b in bufs.items():
        if b.rows == "parts":
            pre = name[:-len("parts")]
            for vec, off in ((pre + "dgamma", 0), (pre + "dbeta", c.D)):
                before[vec] = u[vec].clone()
                jobs.append(o.partial_sum_job(u[name], b.n, u[vec], col_off=off, length=c.D))
    if jobs:
        o.partial_sums(jobs)
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in u.items()}, {k: t.cpu() for k, t in before.items()}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_row_block_launch_against_fp64(gpu, case):
    from musicstyletransfer_amd import ops as o
    c = case
    bufs, _ = R.plan(c)
    ins = R.operands(c)
    got, before = _run(o, c, ins, gpu)
    results = R.check(c, ins, got)
    print(f"\n{c.id}: worst error / bound " + ", ".join(f"{r.name} {r.ratio:.3f}" for r in results))
    failed = [R.describe(c, r) for r in results if r.bad.any()]
    assert not failed, "\n".join(failed)
    assert R.intact(c, got) == []
    for name, t in before.items():  # with partials the launch itself leaves dgamma / dbeta alone
        assert (t[:c.D] == R.INIT).all() and (t[c.D:] == R.SENTINEL).all(), f"{name}: touched by a launch that was given partials"
    if before:  # the partial rows and their sums repeat bit for bit
        again, _ = _run(o, c, ins, gpu)
        for name, b in bufs.items():
            if b.rows == "parts" or name in before:
                assert torch.equal(got[name][:b.n or None].view(torch.int32), again[name][:b.n or None].view(torch.int32)), \
                    f"{name}: not run-to-run identical"
