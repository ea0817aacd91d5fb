"""mst_dec_tail_step: the last decoder layer's row-wise block, the loss launch and the block's backward as consecutive phases of one
launch's workgroups. Everything is a bitwise comparison with the three launches it replaces (mst_proj_ffn_ln_fwd,
mst_gemm_sigmoid_bce_dgrad_ln, mst_ffn_ln_bwd): the same tile per workgroup, the same chunk rotation, the same K order, the same
epilogues. Only the per-sample loss sums (one atomic per workgroup, in arrival order) may differ, in the last bit."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D, F, P = 128, 512, 128
NAN = float("nan")


def _rnd(shape, dev, scale, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def _inputs(gpu, B, T, dtype):
    R = B * (T + 1)
    f32 = torch.float32
    w = dict(att=_rnd((R, D), gpu, 1.0, dtype, 1), x_in=_rnd((R, D), gpu, 1.0, dtype, 2),
             Wp=_rnd((D, D), gpu, 0.09, dtype, 3), bp=_rnd((D,), gpu, 0.1, f32, 4),
             g1=1 + 0.1 * _rnd((D,), gpu, 1.0, f32, 5), be1=_rnd((D,), gpu, 0.1, f32, 6),
             W1=_rnd((F, D), gpu, 0.09, dtype, 7), b1=_rnd((F,), gpu, 0.1, f32, 8),
             W2=_rnd((D, F), gpu, 0.05, dtype, 9), b2=_rnd((D,), gpu, 0.1, f32, 10),
             g3=1 + 0.1 * _rnd((D,), gpu, 1.0, f32, 11), be3=_rnd((D,), gpu, 0.1, f32, 12),
             Wo=_rnd((P, D), gpu, 0.2, dtype, 13), bo=_rnd((P,), gpu, 0.1, f32, 14))
    w["W1t"], w["W2t"], w["Wot"] = w["W1"].t().contiguous(), w["W2"].t().contiguous(), w["Wo"].t().contiguous()
    g = torch.Generator().manual_seed(15)
    w["labels"] = (torch.rand(B * T, P, generator=g) < 0.05).to(torch.uint8).to(gpu)
    w["seed"] = torch.tensor([77, 0, 0, 0], dtype=torch.int64, device=gpu)
    return w


# every buffer the launches store, by the rows it is indexed with: 'phys' b (T + 1) + 1 + t, 'log' b T + t, 'tile' one row per workgroup
OUT = dict(h1=("phys", D), x1=("phys", D), mean1=("phys", 0), rstd1=("phys", 0), a=("phys", F), h2=("phys", D), x2=("phys", D),
           mean2=("phys", 0), rstd2=("phys", 0), dlogits=("log", P), probs=("log", P), dh=("phys", D), dpre=("phys", F), dh1=("phys", D),
           dh1m=("phys", D), parts3=("tile", 2 * D), parts1=("tile", 2 * D))


def _outputs(gpu, B, T, dtype):
    """all NaN: the launches must fill rows 1..T of every sample and leave position 0 and the guard row behind the last row alone"""
    n = dict(phys=B * (T + 1) + 1, log=B * T + 1, tile=B * T // 64 + 1)
    bufs = {}
    for name, (rows, width) in OUT.items():
        dt = torch.float32 if width == 0 or rows == "tile" else dtype
        bufs[name] = torch.full((n[rows], width) if width else (n[rows],), NAN, dtype=dt, device=gpu)
    bufs["loss"] = torch.zeros(B, dtype=torch.float32, device=gpu)
    return bufs


def _run(o, w, u, B, T, drop, ls, dw, gscale, fused, probs):
    R, M, Sd = B * (T + 1), B * T, T + 1
    groups = (T, Sd, 1)
    v = lambda t: t[:R]  # noqa: E731  (the guard row is not part of the operand)
    at = lambda k: dict(dropout_p=drop, dropout_site=20 + k, dropout_seed_ptr=w["seed"]) if drop > 0 else {}  # noqa: E731
    head = dict(att=v(w["att"]), W=w["Wp"], h1=v(u["h1"]), gamma=w["g1"], beta=w["be1"], mean=u["mean1"], rstd=u["rstd1"], N=D, K=D,
                bias=w["bp"], resid=v(w["x_in"]), **at(0))
    fwd = dict(x=v(u["x1"]), W1=w["W1"], a_out=v(u["a"]), W2=w["W2"], h_out=v(u["h2"]), gamma=w["g3"], beta=w["be3"], y_out=v(u["x2"]),
               mean=u["mean2"], rstd=u["rstd2"], ff1=dict(K=D, bias=w["b1"], act=o.ACT_RELU, **at(1)),
               ff2=dict(K=F, bias=w["b2"], self_resid=True, **at(2)), proj=head, row_groups=groups)
    dl, pr = u["dlogits"][:M], (u["probs"][:M] if probs else None)
    loss = dict(A=v(u["x2"]), B=w["Wo"], labels=w["labels"], loss=u["loss"], T=T, dlogits=dl, probs=pr, label_smoothing=ls,
                downweight=dw, gscale=gscale, M=M, K=D, bias=w["bo"], a_remap=groups)
    dgrad = dict(A=dl, B=w["Wot"], dX_out=v(u["dh"]), x=v(u["h2"]), gamma=w["g3"], mean=u["mean2"], rstd=u["rstd2"], dgamma=None, dbeta=None,
                 mask_mode=2, partials=u["parts3"][:M // 64], M=M, N=D, K=P, c_remap=groups, **at(2))
    ln1 = dict(dx_masked=v(u["dh1m"]), mask_mode=1, **at(0)) if drop > 0 else {}
    bwd = dict(dff=v(u["dh"]), W2t=w["W2t"], dpre_out=v(u["dpre"]), gate=v(u["a"]), W1t=w["W1t"], dx_out=v(u["dh1"]), x=v(u["h1"]),
               gamma=w["g1"], mean=u["mean1"], rstd=u["rstd1"], dgamma=None, dbeta=None, alpha=1.0 / (1.0 - drop) if drop > 0 else 1.0,
               partials=u["parts1"][:M // 64], row_groups=groups, **ln1)
    if fused:
        o.dec_tail_step(fwd, loss, dgrad, bwd)
    else:
        o.ffn_ln_fwd(**fwd)
        kw = {k: x for k, x in loss.items() if k not in ("A", "B", "labels", "loss", "T")}
        o.gemm_sigmoid_bce(loss["A"], loss["B"], loss["labels"], loss["loss"], T, dgrad=dgrad, **kw)
        o.ffn_ln_bwd(**bwd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T,dtype,drop,ls,dw,probs", [
    (7, 256, BF, 0.2, 0.1, True, True),              # 28 tiles: xcd_chunk's ragged eighths, all four chunk rotations
    (8, 64, torch.float16, 0.0, 0.0, False, False),  # 8 tiles: a multiple of 8; probabilities left out
    (3, 64, BF, 0.2, 0.0, True, True),               # 3 tiles: fewer than XCDs
], ids=["28tiles", "8tiles", "3tiles"])
def test_dec_tail_step_equals_the_three_launches(gpu, B, T, dtype, drop, ls, dw, probs):
    from musicstyletransfer_amd import ops as o
    w = _inputs(gpu, B, T, dtype)
    gscale = 1024.0 if dtype == torch.float16 else 4.0
    one, three = _outputs(gpu, B, T, dtype), _outputs(gpu, B, T, dtype)
    _run(o, w, one, B, T, drop, ls, dw, gscale, True, probs)
    _run(o, w, three, B, T, drop, ls, dw, gscale, False, probs)
    assert torch.allclose(one["loss"], three["loss"], rtol=1e-6, atol=0), "loss"
    assert (three["loss"] > 0).all()
    for name, (rows, width) in OUT.items():
        a, b = one[name], three[name]
        written = not ((name == "probs" and not probs) or (name == "dh1m" and drop == 0))
        if not written:
            assert a.isnan().all() and b.isnan().all(), name
            continue
        if rows == "phys":
            body = lambda t: t[:-1].view(B, T + 1, -1)[:, 1:]  # noqa: E731
            assert a[:-1].view(B, T + 1, -1)[:, 0].isnan().all(), f"{name}: position-0 rows were written"
        else:
            body = lambda t: t[:-1]  # noqa: E731
        assert a[-1:].isnan().all(), f"{name}: written past the last row"
        assert not body(b).isnan().any(), f"{name}: the three launches left rows unwritten"
        assert torch.equal(body(a), body(b)), name
    assert one["dh1"][:-1].view(B, T + 1, -1)[:, 1:].float().abs().sum() > 0


# ------------------------------------------------------------------------------------------ step level
DIMS = (128, 128, 3, 32, 64, 1, 4, 128, 2, 4)  # decoder: two layers of width 128 (hidden 512), 128 pitches
B_STEP, T_STEP = 3, 64


def _plan(gpu, dec_tail):
    from test_step_gpu import _setup
    O, E, ocfg, ecfg, params, batch, eps = _setup("pianoroll", DIMS, B_STEP, T_STEP, 21, ragged=False)
    ecfg.e_dropout = ecfg.d_dropout = 0.2
    store = E.ParamStore(ecfg, gpu, BF, params_np=params)
    plan = E.StepPlan(store, B_STEP, T_STEP, clip_gradient=1.0, kl_weight=0.5, label_smoothing=0.1, negative_label_downscaling=True)
    plan.LN_PARTIALS_MIN = 0  # one partial row per workgroup, summed in a fixed order: no fp32 atomics reach the gradients
    plan.dec_tail = dec_tail
    plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
    return store, plan


def test_three_adam_steps_with_and_without_the_one_launch_tail(gpu):
    """two plans from the same initial state, Forms.dec_tail on and off: after three captured Adam steps with dropout 0.2 every weight and
    the KL are bit-equal and the reconstruction loss agrees to 1e-6; the captured step has exactly two kernel launches fewer; the
    validation pass (forward + losses without gradient) of the on-plan keeps the three launches and matches the off-plan's"""
    res = {}
    for on in (True, False):
        store, plan = _plan(gpu, on)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
            saved = [t.clone() for t in (store.w, store.m, store.v, store.w16, store.wt16, store.step_state)]
            rng = plan.rng_state.clone()
            plan.step_kernels(True)  # (HIP modules load lazily and are not capturable)
            torch.cuda.synchronize()
            assert plan.forms.dec_tail == on
            plan.capture(True)
            for t, s in zip((store.w, store.m, store.v, store.w16, store.wt16, store.step_state), saved):
                t.copy_(s)
            plan.rng_state.copy_(rng)
            for _ in range(3):
                plan.run()
            torch.cuda.synchronize()
            nodes = plan.graph_nodes()
            step = dict(w=store.w.clone(), kl=plan.kl.clone(), recon=plan.recon.clone(), dec_out=plan.dec_out.clone())
            plan.fwd_bwd_kernels(is_train=False)  # validation: the three launches on either plan
            torch.cuda.synchronize()
            assert not plan.forms.dec_tail
            res[on] = dict(step, nodes=nodes, v_recon=plan.recon.clone(), v_kl=plan.kl.clone(), v_dec_out=plan.dec_out.clone())
    a, b = res[True], res[False]
    assert b["nodes"][1] - a["nodes"][1] == 2 and b["nodes"][0] - a["nodes"][0] == 2, (a["nodes"], b["nodes"])
    assert torch.equal(a["w"], b["w"]) and torch.equal(a["kl"], b["kl"]) and torch.equal(a["dec_out"], b["dec_out"])
    assert torch.allclose(a["recon"], b["recon"], rtol=1e-6, atol=0)
    assert torch.equal(a["v_kl"], b["v_kl"]) and torch.equal(a["v_dec_out"], b["v_dec_out"])
    assert torch.allclose(a["v_recon"], b["v_recon"], rtol=1e-6, atol=0)
    assert (a["recon"] > 0).all() and not a["w"].isnan().any()


def test_forward_alone_fills_dec_out(gpu):
    """plan.forward() without a following losses(with_grad=True) — validation, Model.__call__, diagnostics — keeps the last decoder
    layer's launch: dec_out is what the one-launch step leaves there"""
    store, plan = _plan(gpu, True)
    rng = plan.rng_state.clone()
    plan._tick_adam = False
    plan.forward()
    torch.cuda.synchronize()
    assert not plan.forms.dec_tail
    alone = plan.dec_out.clone()
    plan.dec_out.zero_()
    plan.rng_state.copy_(rng)
    plan.forward(with_grad=True)
    plan.losses(with_grad=True)
    torch.cuda.synchronize()
    assert plan.forms.dec_tail
    assert alone.float().abs().sum() > 0 and torch.equal(plan.dec_out, alone)
