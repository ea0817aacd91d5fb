"""Device-resident training schedules (KL warm-up with optional cycles, free bits, learning-rate warm-up): the schedule block the
step's first launch writes from Adam's step count, the scheduled forms of the latent block's backward launch and of the step-closing
bookkeeping, and whole steps against the constant path given each step's values from engine.schedule_values. Nearly everything is a
bitwise comparison: the scheduled launches are the unscheduled ones with a device word in place of a launch constant."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DIMS = (128, 128, 3, 32, 64, 1, 4, 64, 2, 4)  # the narrow widths of test_step_gpu.test_pianoroll_label_smoothing_downweighting_klweight
B_STEP, T_STEP = 4, 33


def _order_free(plan):
    """At this size a LayerNorm-backward launch has fewer than StepPlan.LN_PARTIALS_MIN workgroups and adds its d gamma / d beta with
    fp32 atomics, in arrival order: two identical runs of the UNSCHEDULED step then differ in the last bits of the decoder's d gamma and
    of Adam's moments (measured, five runs of six steps). The partial-row form — one row per workgroup, summed in a fixed order by the
    weight-gradient flush — has no such freedom (measured: every gradient equal in all five runs), so the bitwise comparisons of whole
    steps select it, on both sides alike."""
    plan.LN_PARTIALS_MIN = 0
    return plan


def _small_step(gpu, seed=13, order_free=True, **hyper):
    """store + plan of the small piano-roll model on a full-length batch, the batch loaded (explicit eps, dropout 0); order_free=False
    keeps the LayerNorm-backward form the product selects at this size"""
    from test_step_gpu import _setup
    O, E, ocfg, ecfg, params, batch, eps = _setup("pianoroll", DIMS, B_STEP, T_STEP, seed, ragged=False)
    store = E.ParamStore(ecfg, gpu, torch.bfloat16, params_np=params)
    plan = E.StepPlan(store, B_STEP, T_STEP, clip_gradient=1.0, **hyper)
    if order_free:
        _order_free(plan)
    plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
    return E, store, plan, (batch, eps)


def _state(store):
    return [t.clone() for t in (store.w, store.m, store.v, store.w16, store.wt16, store.step_state, store._metric_buf)]


def _restore(store, saved):
    for t, s in zip((store.w, store.m, store.v, store.w16, store.wt16, store.step_state, store._metric_buf), saved):
        t.copy_(s)


def _label(o, name, args):
    """an entry point as the call lists name it: mst_adam_flat with what the block it was handed switches on (ops.adam_flat_form)"""
    if name != "mst_adam_flat":
        return name
    form = o.adam_flat_form(args[0])
    return name + "".join("+" + k for k in ("emb", "sched", "gnorm", "ema") if form[k])


def _calls(o, fn):
    """names of the C-ABI entry points fn() goes through, in order (_label)"""
    names, real = [], o.call

    def call(name, *a):
        if name != "mst_adam_flat_form":  # (_label's own question)
            names.append(_label(o, name, a))
        return real(name, *a)

    o.call = call
    try:
        fn()
    finally:
        o.call = real
    return names


# ------------------------------------------------------------------------------------------ a. the schedule block under replay
def test_schedule_block_follows_the_step_count_through_a_captured_graph(gpu):
    """one capture, 15 replays: after each, the block is {beta_t, tau, f_lr, t} of engine.schedule_values bit for bit (t / W is a
    correctly rounded quotient on both sides, beta_t one rounding of a double product) and lr_t carries the warm-up factor"""
    W_b, C, W_lr, tau, klw, lr = 4, 6, 5, 1.5, 0.5, 1e-3
    E, store, plan, _ = _small_step(gpu, lr=lr, kl_weight=klw, kl_warmup_steps=W_b, kl_cycle_steps=C, kl_free_bits=tau, lr_warmup_steps=W_lr)
    assert plan.forms.sched
    saved = _state(store)
    b1, b2 = plan.opt["beta1"], plan.opt["beta2"]
    seen = []
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
        plan.step_kernels(True)  # (HIP modules load lazily and are not capturable)
        torch.cuda.synchronize()
        plan.capture(True)
        _restore(store, saved)  # step count 0 again
        for t in range(1, 16):
            plan.run()
            torch.cuda.synchronize()
            beta, f_lr = E.schedule_values(t, klw, kl_warmup_steps=W_b, kl_cycle_steps=C, lr_warmup_steps=W_lr)
            want = np.array([beta, tau, f_lr, t], np.float32)
            got = store.sched.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (t, got, want)
            assert int(store.step_state[0].item()) == t
            lr_t = float(store.step_state.view(torch.float32)[1].item())
            ref = (lr * f_lr) * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            assert abs(lr_t - ref) <= 1e-6 * ref, (t, lr_t, ref)  # (test_adam_flat_mxnet_rule's relative tolerance on what lr_t scales)
            m = store.read_metrics(reset=False)
            assert m["kl_weight"] == float(np.float32(beta)) and m["lr_scale"] == float(np.float32(f_lr))
            seen.append(beta)
    assert seen[3] == seen[5] == klw and seen[6] == seen[0] == seen[12] == klw / 4  # plateau, restarts at t = 7 and 13
    assert int(store.step_status.cpu()[1]) == 0  # no step was skipped


# ------------------------------------------------------------------------------------------ b. latent backward
@pytest.mark.parametrize("proj", [False, True], ids=["read", "proj"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,De,Z,Dd", [(5, 256, 64, 128), (3, 256, 256, 128)], ids=["preloaded", "general"])
def test_latent_bwd_sched_selects_per_sample_between_the_beta_and_the_zero_launch(gpu, B, De, Z, Dd, dtype, proj):
    """the workgroup of sample b owns that sample's rows: with kl_b above the allowance they are the rows of the unscheduled launch
    at kl_weight = beta, otherwise those of the launch at kl_weight = 0 — bit for bit"""
    from musicstyletransfer_amd import ops as o
    g = torch.Generator().manual_seed(5 + B + Z)
    r = lambda *sh, sc=1.0, dt=torch.float32: (torch.randn(*sh, generator=g) * sc).to(dt).to(gpu)
    S, Sd, Cn, nq = 3, 4, 3, 3 * Dd
    Wl, Wh, eps = r(2 * Z, De, sc=0.2), r(Dd, Z, sc=0.3), r(B, Z)
    # per-sample spread of mu: KLs far apart (about 0.5 Z scale_b^2 each)
    scale = torch.tensor([0.4 + 0.35 * b for b in range(B)]).view(B, 1)
    mu = ((torch.randn(B, Z, generator=g)) * scale).to(gpu)
    sigma = (1.0 + 0.2 * torch.randn(B, Z, generator=g)).clamp(min=0.3).to(gpu)
    kl = (0.5 * (sigma * sigma + mu * mu - 1 - torch.log(sigma * sigma)).sum(1)).contiguous()
    classes = torch.tensor([b % Cn for b in range(B)], dtype=torch.int32, device=gpu)
    g0 = r(B, Sd, Dd, sc=0.1, dt=dtype)
    dq3, Wt, r3 = r(B, Sd, nq, sc=0.1, dt=dtype), r(Dd, nq, sc=0.1, dt=dtype), r(B, Sd, Dd, sc=0.1, dt=dtype)
    alpha_d, beta = math.sqrt(Dd), 0.375
    ks = np.sort(kl.cpu().numpy())
    tau = float(np.float32(0.5 * (ks[B // 2 - 1] + ks[B // 2])))
    above = (kl > tau).cpu().numpy()
    assert above.any() and (~above).any() and (np.abs(ks - tau) > 1e-3 * tau).all(), (ks, tau)

    def run(kl_weight=0.0, sched=None):
        dcls = torch.zeros(Cn, Dd, device=gpu)
        denc = torch.zeros(B, S, De, dtype=dtype, device=gpu)
        scratch = torch.zeros(B * (Dd + 2 * Z), device=gpu)
        o.latent_bwd_vec(Wl, eps, Wh, classes, mu, sigma, g0, alpha_d, kl_weight, 1.0, dcls, denc, scratch,
                         proj=(dq3, Wt, r3) if proj else None, sched=sched)
        torch.cuda.synchronize()
        return dict(tvec=scratch[: B * Dd].view(B, Dd).clone(), dlat=scratch[B * Dd:].view(B, 2 * Z).clone(), denc0=denc[:, 0].clone(),
                    denc_rest=denc[:, 1:].clone(), dcls=dcls)

    at_beta, at_zero = run(beta), run(0.0)
    assert not torch.equal(at_beta["dlat"], at_zero["dlat"])
    block = lambda t_: torch.tensor([beta, t_, 1.0, 3.0], device=gpu)
    got = run(kl_weight=123.0, sched=(block(tau), kl))  # (kl_weight is ignored by the scheduled form)
    for b in range(B):
        want = at_beta if above[b] else at_zero
        for k in ("tvec", "dlat", "denc0"):
            assert torch.equal(got[k][b], want[k][b]), (k, b, bool(above[b]))
    assert torch.equal(got["dcls"], at_beta["dcls"]) and not got["denc_rest"].any()
    got = run(sched=(block(0.0), kl))  # tau = 0: every sample is charged
    for k in ("tvec", "dlat", "denc0", "dcls"):
        assert torch.equal(got[k], at_beta[k]), k
    # strictly above: a sample exactly AT the allowance is not charged
    b_eq = int(np.argmax(above))
    got = run(sched=(block(float(kl[b_eq].item())), kl))
    assert torch.equal(got["dlat"][b_eq], at_zero["dlat"][b_eq])


# ------------------------------------------------------------------------------------------ c. bookkeeping
@pytest.mark.parametrize("emb", [False, True], ids=["adam_flat", "adam_flat_emb"])
def test_adam_sched_bookkeeping_equals_the_constant_launch_on_a_precharged_kl(gpu, emb):
    from musicstyletransfer_amd import _lib, ops as o
    BF = torch.bfloat16
    n, B, beta, tau = 4096 + 3, 7, 0.375, 3.0
    g = torch.Generator().manual_seed(77)
    w0, grad = torch.randn(n, generator=g).to(gpu), (torch.randn(n, generator=g) * 50).to(gpu)
    recon, kl = (torch.rand(B, generator=g) * 20).to(gpu), (torch.rand(B, generator=g) * 8).to(gpu)
    charged = (kl - tau).clamp(min=0.0)  # fp32, one subtraction: what the scheduled launch forms per sample
    assert (charged > 0).any() and (charged == 0).any()
    sched = torch.tensor([beta, tau, 1.0, 6.0], device=gpu)
    word = torch.tensor([48], dtype=torch.int32, device=gpu)
    rows, cols, so = 10, 32, 64
    ld_t = o.roundup(rows, 8)

    def run(scheduled, status=None, expect_val=48, t0=5):
        t = dict(w=w0.clone(), m=torch.zeros(n, device=gpu), v=torch.zeros(n, device=gpu), w16=torch.zeros(n, dtype=BF, device=gpu),
                 wt16=torch.zeros(cols * ld_t, dtype=BF, device=gpu), total=torch.zeros(B, device=gpu), metric=torch.zeros(3, device=gpu))
        t["state"] = torch.tensor([t0, 0], dtype=torch.int32, device=gpu)
        t["state"].view(torch.float32)[1] = 1e-3
        guard = dict(status=status, expect=[(word, expect_val)]) if status is not None else {}
        mt = dict(recon=recon, kl=kl if scheduled else charged, kl_weight=99.0 if scheduled else beta, total=t["total"], metric=t["metric"], **guard)
        o.adam_flat(t["w"], grad, t["m"], t["v"], t["w16"], t["state"], lr=1e-3, rescale=1 / 32, clip=1.0, advance_step=False, metrics=mt,
                    emb=dict(base=0, specs=[(so, 0, rows, cols)], wt16=t["wt16"]) if emb else None, sched=sched if scheduled else None)
        torch.cuda.synchronize()
        return t

    a, b = run(True), run(False)
    for k in ("w", "m", "v", "w16", "wt16", "total"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["w"], w0) and (not emb or a["wt16"].any())
    assert torch.allclose(a["total"], recon + beta * charged, rtol=1e-6, atol=0)
    # the running sums: [0] the RAW KL (the plain launch on the raw vector forms the same sum in the same order), [1] the charged total
    raw = torch.zeros(3, device=gpu)
    o.loss_combine(recon, kl, beta, None, raw)
    torch.cuda.synchronize()
    assert a["metric"][0].item() == raw[0].item() and abs(a["metric"][0].item() - kl.double().sum().item()) <= 1e-5 * kl.sum().item()
    assert a["metric"][1].item() == b["metric"][1].item() and a["metric"][2].item() == B
    # a raised guard word: weights, moments and sums untouched, the step count taken back, the skip counted
    status = torch.zeros(3, dtype=torch.int32, device=gpu)
    t = run(True, status=status, expect_val=47)
    assert torch.equal(t["w"], w0) and not t["m"].any() and not t["v"].any() and not t["metric"].any() and not t["total"].any()
    assert status.tolist()[:2] == [_lib.STEP_INCOMPLETE, 1] and int(t["state"][0].item()) == 4
    t = run(True, status=status, expect_val=48)  # sticky
    assert torch.equal(t["w"], w0) and not t["metric"].any() and status.tolist()[:2] == [_lib.STEP_INCOMPLETE, 2]
    status.zero_()
    t = run(True, status=status, expect_val=48)  # healthy again: the update and the sums are taken
    assert torch.equal(t["w"], a["w"]) and torch.equal(t["metric"], a["metric"]) and status.tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------ d. whole steps
def _six_steps(gpu, tau, ref_weight):
    """six captured scheduled steps (W_b 4, W_lr 3) and six steps of unscheduled plans at kl_weight = ref_weight(beta_t), lr = lr * f_lr(t),
    both from the same weights; -> per step (scheduled weights, reference weights, scheduled plan's kl)"""
    W_b, W_lr, klw, lr = 4, 3, 0.5, 1e-3
    E, sa, pa, (batch, eps) = _small_step(gpu, lr=lr, kl_weight=klw, kl_warmup_steps=W_b, lr_warmup_steps=W_lr, kl_free_bits=tau)
    saved = _state(sa)
    out = []
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
        pa.step_kernels(True)
        torch.cuda.synchronize()
        pa.capture(True)
        _restore(sa, saved)
        sb = E.ParamStore(sa.cfg, gpu, torch.bfloat16, params_np=sa.to_numpy("w"))
        assert torch.equal(sa.w, sb.w) and torch.equal(sa.wt16, sb.wt16) and torch.equal(sa.w16, sb.w16)
        for t in range(1, 7):
            pa.run()
            beta, f_lr = E.schedule_values(t, klw, kl_warmup_steps=W_b, lr_warmup_steps=W_lr)
            pb = _order_free(E.StepPlan(sb, B_STEP, T_STEP, clip_gradient=1.0, lr=lr * f_lr, kl_weight=ref_weight(beta)))
            assert not pb.forms.sched
            pb.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
            pb.step_kernels(True)
            torch.cuda.synchronize()
            assert int(sa.step_state[0].item()) == int(sb.step_state[0].item()) == t
            out.append((sa.w.clone(), sb.w.clone(), pa.kl.clone(), pa.total.clone(), pb.total.clone()))
    assert int(sa.step_status.cpu()[1]) == 0 and int(sb.step_status.cpu()[1]) == 0
    return out


def _report(out, what):
    lines = []
    for t, (wa, wb, _, ta, tb) in enumerate(out, 1):
        d = (wa - wb).abs()
        lines.append(f"{what} step {t}: {int((wa != wb).sum())} of {wa.numel()} weights differ (max {float(d.max()):.3g}); totals equal: {torch.equal(ta, tb)}")
    print("\n".join(lines))
    return lines


def test_scheduled_steps_equal_constant_steps_given_each_steps_values(gpu):
    out = _six_steps(gpu, 0.0, lambda beta: beta)
    lines = _report(out, "tau 0")
    for t, (wa, wb, _, ta, tb) in enumerate(out, 1):
        assert torch.equal(wa, wb), "\n".join(lines)


def test_free_bits_above_every_kl_equal_constant_steps_at_weight_zero(gpu):
    out = _six_steps(gpu, 1e6, lambda beta: 0.0)
    lines = _report(out, "tau above every KL")
    assert all(float(kl.max()) < 1e6 for _, _, kl, _, _ in out)
    for t, (wa, wb, _, ta, tb) in enumerate(out, 1):
        assert torch.equal(wa, wb), "\n".join(lines)


@pytest.mark.parametrize("tau,ref_weight", [(0.0, lambda beta: beta), (1e6, lambda beta: 0.0)], ids=["tau0", "tau_above_every_kl"])
def test_scheduled_steps_on_the_default_layernorm_form_meet_the_step_thresholds(gpu, tau, ref_weight):
    """The two tests above assert bit-identity on the partial-sum LayerNorm-backward form only (_order_free). The form the product
    selects at this size adds d gamma / d beta with fp32 atomics, so the unscheduled step is not bit-identical to ITSELF there; on
    that form the scheduled step is held to the thresholds tests/test_step_gpu.py::_compare_step applies to a bf16 step on fewer than
    4096 rows, against the unscheduled step given the step's values, each step from identical weights, moments and step count."""
    from test_step_gpu import _cos
    W_b, W_lr, klw, lr = 4, 3, 0.5, 1e-3
    E, sa, pa, (batch, eps) = _small_step(gpu, order_free=False, lr=lr, kl_weight=klw, kl_warmup_steps=W_b, lr_warmup_steps=W_lr, kl_free_bits=tau)
    assert pa.LN_PARTIALS_MIN == E.StepPlan.LN_PARTIALS_MIN and pa.forms.sched
    grad_cos, noisy_cos, global_cos, max_err, elbo_tol = 0.96, 0.6, 0.985, 0.6, 2e-3  # (_compare_step: small, bf16)
    noisy = lambda n: ".att.W_k." in n or ".att.W_q." in n or n.startswith("decoder.latent2hid") or n == "decoder.class2hid.weight"
    rel = lambda a, b: abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)
    saved, bad = _state(sa), []
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        pa.step_kernels(True)
        torch.cuda.synchronize()
        pa.capture(True)
        _restore(sa, saved)
        sb = E.ParamStore(sa.cfg, gpu, torch.bfloat16, params_np=sa.to_numpy("w"))
        for t in range(1, 7):
            for dst, src in zip((sb.w, sb.m, sb.v, sb.w16, sb.wt16, sb.step_state), (sa.w, sa.m, sa.v, sa.w16, sa.wt16, sa.step_state)):
                dst.copy_(src)  # identical state in, as _compare_step gives its oracle
            pa.run()
            beta, f_lr = E.schedule_values(t, klw, kl_warmup_steps=W_b, lr_warmup_steps=W_lr)
            pb = E.StepPlan(sb, B_STEP, T_STEP, clip_gradient=1.0, lr=lr * f_lr, kl_weight=ref_weight(beta))
            pb.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
            pb.step_kernels(True)
            torch.cuda.synchronize()
            assert int(sa.step_state[0].item()) == int(sb.step_state[0].item()) == t
            for nm, a, b, tol in (("recon", pa.recon, pb.recon, 1e-3), ("ELBO", pa.total, pb.total, elbo_tol), ("KL", pa.kl, pb.kl, elbo_tol)):
                if not rel(a.mean(), b.mean()) <= tol:
                    bad.append(f"step {t} {nm} mean {float(a.mean()):.6f} vs {float(b.mean()):.6f}")
            ga, gb, wa, wb = sa.to_numpy("g"), sb.to_numpy("g"), sa.to_numpy("w"), sb.to_numpy("w")
            gmax = max(float(np.abs(r).max()) for r in gb.values())
            num = den_a = den_b = 0.0
            for name, rg in gb.items():
                gg = ga[name]
                if np.abs(rg).max() > 1e-4 * gmax:
                    c = _cos(gg, rg)
                    if not c >= (noisy_cos if noisy(name) else grad_cos):
                        bad.append(f"step {t} gradient of {name}: cosine {c:.4f}")
                    ratio = float(np.linalg.norm(gg.astype(np.float64)) / max(np.linalg.norm(rg.astype(np.float64)), 1e-300))
                    slack = 0.25 + (math.sqrt(max(0.0, 1.0 - min(c, 1.0) ** 2)) if noisy(name) else 0.0)
                    if not 1.0 / (1.0 + slack) <= ratio <= 1.0 + slack:
                        bad.append(f"step {t} gradient of {name}: norm ratio {ratio:.3f}")
                    if not noisy(name) and not np.abs(gg - rg).max() <= max_err * float(np.abs(rg).max()):
                        bad.append(f"step {t} gradient of {name}: max err {np.abs(gg - rg).max():.3g}")
                    sure = np.abs(rg) > 0.5 * np.abs(rg).max()
                    if not noisy(name) and not np.abs(wa[name] - wb[name])[sure].max() <= 0.25 * lr:
                        bad.append(f"step {t} {name}: updated weights differ by {np.abs(wa[name] - wb[name])[sure].max():.3g}")
                elif not np.abs(gg - rg).max() <= 2e-3 * gmax:
                    bad.append(f"step {t} gradient of {name} (~0 in the reference): {np.abs(gg).max():.3g}")
                num += float((gg.astype(np.float64) * rg).sum())
                den_a += float((gg.astype(np.float64) ** 2).sum())
                den_b += float((rg.astype(np.float64) ** 2).sum())
            if not num / math.sqrt(den_a * den_b) >= global_cos:
                bad.append(f"step {t} global gradient cosine {num / math.sqrt(den_a * den_b):.5f}")
            print(f"default LN form, step {t}: global gradient cosine {num / math.sqrt(den_a * den_b):.7f}, "
                  f"{sum(int((wa[n] != wb[n]).sum()) for n in wa)} weights differ")
    assert int(sa.step_status.cpu()[1]) == 0 and int(sb.step_status.cpu()[1]) == 0
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------ e. resume
def test_schedule_resumes_with_the_optimizer_state(gpu, tmp_path):
    from music_style_transfer.VarAutoEncoder import main
    from musicstyletransfer_amd import engine as E
    folder = str(tmp_path / "toy")
    flags = ["--toy", "--gpu", "--max-steps", "3", "--kl-warmup-steps", "8", "--model-output", folder]
    t = main.main(flags)
    assert t.config.kl_warmup_steps == 8 and t._last_plan.forms.sched
    assert t.model.store.read_metrics(reset=False)["kl_weight"] == E.schedule_values(3, 1.0, kl_warmup_steps=8)[0]
    t._checkpoint(os.path.join(folder, "model"), None)
    t2 = main.main(flags)  # a fresh Trainer: resumes at n_batches = 3 and runs one step
    assert t2.train_state.n_batches == 4 and int(t2.model.store.step_state[0].item()) == 4
    m = t2.model.store.read_metrics(reset=False)
    assert m["kl_weight"] == E.schedule_values(4, 1.0, kl_warmup_steps=8)[0] == 0.5 and m["lr_scale"] == 1.0
    got = t2.collect_metrics()
    assert got["kl_weight"] == 0.5 and got["lr_scale"] == 1.0 and np.isfinite(got["total_loss"])


# ------------------------------------------------------------------------------------------ f. defaults are the old path
def test_defaults_resolve_to_the_plain_launches(gpu):
    from musicstyletransfer_amd import ops as o
    E, sa, pa, (batch, eps) = _small_step(gpu, lr=1e-3, kl_weight=0.5)  # built without the new keywords
    _, sb, pb, _ = _small_step(gpu, lr=1e-3, kl_weight=0.5, kl_warmup_steps=0, kl_cycle_steps=0, kl_free_bits=0.0, lr_warmup_steps=0)
    _, sc, pc, _ = _small_step(gpu, lr=1e-3, kl_weight=0.5, kl_warmup_steps=4, kl_free_bits=2.0, lr_warmup_steps=3)
    assert not pa.forms.sched and not pb.forms.sched and not pb.scheduled and pc.forms.sched
    names = {}
    for key, plan, store in (("a", pa, sa), ("b", pb, sb), ("c", pc, sc)):
        names[key] = _calls(o, lambda: plan.step_kernels(True))
        plan.step_kernels(True)
        torch.cuda.synchronize()
    assert torch.equal(sa.w, sb.w) and torch.equal(sa.m, sb.m) and torch.equal(sa.v, sb.v) and torch.equal(pa.kl, pb.kl)
    scheduled = lambda n: n.endswith("_sched") or "+sched" in n  # (the latent backward by its name, Adam by its label)
    plain = lambda n: n[: -len("_sched")] if n.endswith("_sched") else n.replace("+sched", "")
    assert names["a"] == names["b"] and not any(scheduled(n) for n in names["a"])
    assert not sb.sched.any() and "kl_weight" not in sb.read_metrics(reset=False)  # nothing wrote the block
    assert pb.metrics(reset=False)["kl_weight"] == 0.5 and pb.metrics(reset=False)["lr_scale"] == 1.0
    # the scheduled step adds no launch: the same entry points in the same order, two of them in their scheduled form (each issues
    # the launches of its unscheduled sibling)
    assert [plain(n) for n in names["c"]] == names["a"]
    assert [plain(n) for n in names["c"] if scheduled(n)] == [
        n for n in names["a"] if n.startswith("mst_latent_bwd_vec") or n.startswith("mst_adam_flat")]
    two = [n for n in names["c"] if scheduled(n)]
    assert len(two) == 2 and two[0].startswith("mst_latent_bwd_vec") and two[0].endswith("_sched")
    assert two[1].startswith("mst_adam_flat+") and two[1].endswith("+sched") and sum(n.startswith("mst_adam_flat") for n in names["c"]) == 1
    # ... and the captured graphs say the same of the launches themselves: as many nodes, as many kernel launches among them
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
        counts = [plan.capture(True).graph_nodes() for plan in (pa, pb, pc)]
    torch.cuda.synchronize()
    assert counts[0] == counts[1] == counts[2] and 0 < counts[0][1] <= counts[0][0], counts
    # a validation step keeps the constants: full kl_weight, no free bits, and it does not touch the block
    block = sc.sched.clone()
    pc.step_kernels(False)
    torch.cuda.synchronize()
    assert torch.equal(sc.sched, block) and torch.equal(pc.total, pc.recon + 0.5 * pc.kl)
