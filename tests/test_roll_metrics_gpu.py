"""The piano-roll counts {tp, pred, pos, cells} every BCE launch can keep (mst_bce_args.counts, mst_sigmoid_bce_counts) on a real
MI355X: mst_sigmoid_bce_counts (4- and 8-wide sweeps, NaN pad columns, two workgroups per sample), mst_gemm_sigmoid_bce (both tile
widths, two column tiles, forward only) and _dgrad_ln (one launch and two), mst_dec_tail_step, and the trainer's metrics on top of them.
Every count comparison is EXACT integer equality against numpy on the 16-bit logits the launch consumed or stored ("predicted" is:
that logit > 0); every other output of a counting launch is bit-identical to the same launch without counts. The operands are those
of tests/loss_refs.py."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_refs as L  # noqa: E402

pytestmark = pytest.mark.gpu
S = L.SENTINEL
SLOTS = 256
GUARD = 0x5A5A5A5A5A5A5A5A
BCE_IDS = ("p30-bytes", "p36-4byte", "p128-wide", "p128-ld132")
FUSED_IDS = ("bn128", "bn256-dw", "bn256x2-alpha", "bn128-forward", "dgrad-one", "dgrad-two-p256")
BCE_RUNS = [(L.BCE_CASE[i], d, m) for i in BCE_IDS for d in L.DTYPES for m in L.BCE_CASE[i].modes]
FUSED_RUNS = [(L.FUSED_CASE[i], d, m) for i in FUSED_IDS for d in L.DTYPES for m in L.FUSED_CASE[i].modes]
_id = lambda r: f"{r[0].id}-{L.DT_NAME[r[1]]}-{r[2]}"  # noqa: E731


def test_the_case_tables_offer_what_this_file_relies_on():
    assert L.BCE_CASE["p30-bytes"].form[:2] == (4, 1) and L.BCE_CASE["p36-4byte"].form[:2] == (4, 4)
    assert L.BCE_CASE["p128-wide"].form == (8, 8, 8, 8, 2) and L.BCE_CASE["p128-ld132"].form[0] == 4
    assert "known" in L.BCE_CASE["p128-wide"].modes and "known" in L.BCE_CASE["p128-ld132"].modes
    assert [L.FUSED_CASE[i].form for i in FUSED_IDS] == [(128, 1, 0), (256, 1, 0), (256, 2, 0), (128, 1, 0), (128, 1, 1), (256, 1, 2)]


class Counts:
    """the [256, 4] int64 accumulator, zeroed, between two guard stretches of one allocation"""

    def __init__(self, gpu):
        self.flat = torch.full((8 + SLOTS * 4 + 8,), GUARD, dtype=torch.int64, device=gpu)
        self.t = self.flat[8:8 + SLOTS * 4].view(SLOTS, 4)
        self.t.zero_()
        assert self.t.data_ptr() % 16 == 0

    def read(self, what):
        h = self.flat.cpu()
        assert (h[:8] == GUARD).all() and (h[-8:] == GUARD).all(), f"{what}: a store in front of or behind the counts"
        return h[8:-8].view(SLOTS, 4).numpy().copy()


def roll_ref(logits16, labels, P):
    """numpy on the 16-bit logits [M, >= P] and the labels [M, P] -> int64 [tp, pred, pos, cells]"""
    x = logits16[:, :P].float().numpy()
    with np.errstate(invalid="ignore"):
        pred = x > 0
    lab = labels.numpy() == 1
    return np.array([(pred & lab).sum(), pred.sum(), lab.sum(), x.size], dtype=np.int64)


class Guarded:
    """an output of `rows` x `width` at leading dimension ld, `off` elements into a sentinel-filled allocation"""

    def __init__(self, rows, ld, dtype, gpu, off=0):
        self.flat = torch.full((off + (rows + 2) * ld + 8,), S, dtype=dtype, device=gpu)
        self.t = self.flat[off:off + (rows + 2) * ld].view(rows + 2, ld)


def _same_bits(a, b):
    return torch.equal(a.flat.view(torch.uint8), b.flat.view(torch.uint8))


# ------------------------------------------------------------------------------------------ mst_sigmoid_bce_counts
def _run_bce(o, c, dev, dtype, gpu, counts, out=None):
    M = c.B * c.T
    if out is None:
        out = dict(probs=Guarded(M, c.ldp, dtype, gpu, c.off_p), dlogits=Guarded(M, c.ldd, dtype, gpu, c.off_d),
                   loss=Guarded(1, c.B, torch.float32, gpu), npos=torch.full((c.B + 2,), -7, dtype=torch.int32, device=gpu))
    o.sigmoid_bce(dev["logits"], dev["labels"], out["loss"].t[0], c.B, c.T, c.P, label_smoothing=c.ls, downweight=c.dw, npos=out["npos"],
                  probs=out["probs"].t, dlogits=out["dlogits"].t, gscale=c.gscale, pre_zeroed=False, counts=counts)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("run", BCE_RUNS, ids=_id)
def test_sigmoid_bce_counts(gpu, run):
    from musicstyletransfer_amd import ops as o
    c, dtype, mode = run
    what = f"sigmoid_bce_counts {c.id} {L.DT_NAME[dtype]} {mode}"
    host = L.bce_operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    gx = o.sigmoid_bce_form(dtype, c.B, c.T, c.P, dev["logits"], c.ld, dev["labels"], c.ls, c.dw, 1 << 20, 1 << 20, 1 << 20, c.ldp, 1 << 20,
                            c.ldd, c.gscale, False)["gx"]
    assert gx == c.form[4]
    plain = _run_bce(o, c, dev, dtype, gpu, None)
    cnt = Counts(gpu)
    got = _run_bce(o, c, dev, dtype, gpu, cnt.t)
    once = cnt.read(what)
    _run_bce(o, c, dev, dtype, gpu, cnt.t, out=got)
    twice = cnt.read(what)

    want = roll_ref(host["logits"], host["labels"], c.P)
    print(f"\n{what}: counts {once.sum(0).tolist()}, want {want.tolist()}; slots used {int((once[:, 3] != 0).sum())} of {gx * c.B} workgroups")
    assert np.array_equal(once.sum(0), want), f"{what}: counts {once.sum(0).tolist()}, want {want.tolist()}"
    assert want[3] == c.B * c.T * c.P and (host["logits"][:, c.P:].isnan().all())   # the pad columns hold NaN and are no cells
    if mode == "known":
        assert want[1] == 0 and once[:, :2].sum() == 0, f"{what}: a logit of 0 counted as predicted"
    else:
        assert 0 < want[0] < want[1] < want[3] and want[0] < want[2]
    assert np.array_equal(twice, 2 * once), f"{what}: a second launch into the same buffer did not add the same counts again"
    assert not once[gx * c.B:].any(), f"{what}: a slot beyond the grid's {gx * c.B} workgroups was written"
    # the launch stores what it stores without counts
    for k in ("probs", "dlogits") + (("loss",) if gx == 1 else ()):
        assert _same_bits(plain[k], got[k]), f"{what}: {k} differs from the launch without counts"
    assert torch.equal(plain["npos"], got["npos"])


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: L.DT_NAME[d])
@pytest.mark.parametrize("P", [8, 6], ids=["8wide", "4wide-ragged"])
def test_zeros_nan_and_infinities_are_not_predicted(gpu, dtype, P):
    """+0, -0, NaN, the smallest positive and negative values, +inf, -inf, 1: predicted are the positive ones, whatever their size"""
    from musicstyletransfer_amd import ops as o
    tiny = float(torch.finfo(dtype).smallest_normal) * 2.0 ** -(7 if dtype == torch.bfloat16 else 10)   # the smallest subnormal
    row = torch.tensor([0.0, -0.0, float("nan"), tiny, -tiny, float("inf"), float("-inf"), 1.0]).to(dtype)
    assert float(row[3]) > 0 and float(row[4]) < 0
    B, T = 2, 3
    logits = row.repeat(B * T, 1).to(gpu)
    labels = torch.ones(B * T, P, dtype=torch.uint8)
    labels[:, 5] = 0
    cnt = Counts(gpu)
    loss = torch.zeros(B, dtype=torch.float32, device=gpu)
    assert o.sigmoid_bce_form(dtype, B, T, P, logits, 8, 1 << 20, loss=loss)["vec"] == (8 if P == 8 else 4)
    o.sigmoid_bce(logits, labels.to(gpu), loss, B, T, P, counts=cnt.t)
    torch.cuda.synchronize()
    got = cnt.read("special values").sum(0)
    want = roll_ref(row.repeat(B * T, 1), labels, P)
    assert want.tolist() == [B * T * (2 if P == 8 else 1), B * T * (3 if P == 8 else 2), B * T * (P - 1), B * T * P]
    assert np.array_equal(got, want), (got, want)


# ------------------------------------------------------------------------------------------ the fused launches
def _run_fused(o, c, dev, dtype, gpu, counts):
    M, P, K, Sd = c.M, c.P, c.K, c.T + 1
    g = lambda rows, ld, dt=dtype: Guarded(rows, ld, dt, gpu)  # noqa: E731
    out = dict(dlogits=g(M, P + 8) if c.with_c else None, probs=g(M, P + 8) if c.with_probs else None, logits=g(M, P + 8),
               loss=Guarded(1, c.B, torch.float32, gpu))
    out["loss"].t[0].zero_()
    kw = dict(dlogits=None if out["dlogits"] is None else out["dlogits"].t, probs=None if out["probs"] is None else out["probs"].t,
              logits=out["logits"].t, label_smoothing=c.ls, downweight=c.dw, gscale=c.gscale, M=M, K=K, bias=dev["bias"], alpha=c.alpha,
              a_remap=(c.T, Sd, 1), counts=counts)
    dgrad = None
    if c.dgrad:
        parts = o.gemm_nt_ln_parts(M)
        out.update(dx=g(c.B * Sd, K + 8), parts=g(parts, 2 * K, torch.float32), dgamma=g(1, K, torch.float32), dbeta=g(1, K, torch.float32))
        dgrad = dict(A=out["dlogits"].t, B=dev["Wt"], dX_out=out["dx"].t, x=dev["h"], gamma=dev["gamma"], mean=dev["mean"], rstd=dev["rstd"],
                     dgamma=out["dgamma"].t[0], dbeta=out["dbeta"].t[0], mask_mode=2, partials=out["parts"].t[:parts], M=M, N=K, K=P,
                     c_remap=(c.T, Sd, 1))
    o.gemm_sigmoid_bce(dev["x"], dev["W"], dev["labels"], out["loss"].t[0], c.T, dgrad=dgrad, **kw)
    torch.cuda.synchronize()
    return out, kw, dgrad


@pytest.mark.parametrize("run", FUSED_RUNS, ids=_id)
def test_gemm_sigmoid_bce_counts(gpu, run):
    from musicstyletransfer_amd import ops as o
    c, dtype, mode = run
    what = f"gemm_sigmoid_bce counts {c.id} {L.DT_NAME[dtype]} {mode}"
    host = L.fused_operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    plain, _, _ = _run_fused(o, c, dev, dtype, gpu, None)
    cnt = Counts(gpu)
    got, kw, dgrad = _run_fused(o, c, dev, dtype, gpu, cnt.t)
    once = cnt.read(what)
    g, q = o._gemm_bce_args(dev["x"], dev["W"], dev["labels"], got["loss"].t[0], c.T, **kw)
    g2, l = o._gemm_ln_bwd_args(**dgrad) if dgrad else (None, None)
    f = o.gemm_sigmoid_bce_form(g, q, g2, l)
    f = (f["BN"], f["col_tiles"], f["launches"])
    assert f == c.form, f"{what}: the launch takes {f}, the case is meant for {c.form}"   # (the form query does not change with counts)
    M, P = c.M, c.P
    lg16 = got["logits"].t.cpu()[:M, :P]
    want = roll_ref(lg16, host["labels"], P)
    print(f"\n{what}: form {f}; counts {once.sum(0).tolist()}, want {want.tolist()}")
    assert np.array_equal(once.sum(0), want), f"{what}: counts {once.sum(0).tolist()}, want {want.tolist()}"
    if mode == "known":
        assert (lg16 == 0).all() and want[1] == 0
    else:
        assert 0 < want[0] < want[1] < want[3] == M * P
    wgs = (M // 64) * f[1]
    assert not once[wgs:].any(), f"{what}: a slot beyond the grid's {wgs} workgroups was written"
    assert (once[:wgs, 3] == 64 * f[0]).all(), f"{what}: every workgroup counts its own 64 x {f[0]} tile: {once[:wgs, 3].tolist()}"
    # workgroup w holds row block xcd_chunk(w / col_tiles), column tile w % col_tiles; its counts are that tile's
    lab = host["labels"].numpy() == 1
    with np.errstate(invalid="ignore"):
        pred = lg16.float().numpy() > 0
    tiles = sorted((int((pred[r:r + 64, n:n + f[0]] & lab[r:r + 64, n:n + f[0]]).sum()), int(pred[r:r + 64, n:n + f[0]].sum()),
                    int(lab[r:r + 64, n:n + f[0]].sum())) for r in range(0, M, 64) for n in range(0, P, f[0]))
    assert sorted(map(tuple, once[:wgs, :3].tolist())) == tiles, f"{what}: the slots do not hold the tiles' counts"
    _run_fused(o, c, dev, dtype, gpu, cnt.t)
    assert np.array_equal(cnt.read(what), 2 * once), f"{what}: a second launch into the same buffer did not add the same counts again"
    # every other output as without counts
    one_atomic = c.T == 64 and f[1] == 1
    for k, v in got.items():
        if v is not None and (k != "loss" or one_atomic):
            assert _same_bits(v, plain[k]), f"{what}: {k} differs from the launch without counts"


# ------------------------------------------------------------------------------------------ mst_dec_tail_step
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
    return w


OUT = dict(h1=("phys", D), x1=("phys", D), mean1=("phys", 0), rstd1=("phys", 0), a=("phys", F), h2=("phys", D), x2=("phys", D),
           mean2=("phys", 0), rstd2=("phys", 0), dlogits=("log", P), probs=("log", P), logits=("log", P), dh=("phys", D), dpre=("phys", F),
           dh1=("phys", D), parts3=("tile", 2 * D), parts1=("tile", 2 * D))


def _outputs(gpu, B, T, dtype):
    n = dict(phys=B * (T + 1) + 1, log=B * T + 1, tile=B * T // 64 + 1)
    bufs = {}
    for name, (rows, width) in OUT.items():
        dt = torch.float32 if width == 0 or rows == "tile" else dtype
        bufs[name] = torch.full((n[rows], width) if width else (n[rows],), NAN, dtype=dt, device=gpu)
    bufs["loss"] = torch.zeros(B, dtype=torch.float32, device=gpu)
    return bufs


def _run_tail(o, w, u, B, T, ls, dw, gscale, fused, counts):
    R, M, Sd = B * (T + 1), B * T, T + 1
    groups = (T, Sd, 1)
    v = lambda t: t[:R]  # noqa: E731  (the guard row is not part of the operand)
    head = dict(att=v(w["att"]), W=w["Wp"], h1=v(u["h1"]), gamma=w["g1"], beta=w["be1"], mean=u["mean1"], rstd=u["rstd1"], N=D, K=D,
                bias=w["bp"], resid=v(w["x_in"]))
    fwd = dict(x=v(u["x1"]), W1=w["W1"], a_out=v(u["a"]), W2=w["W2"], h_out=v(u["h2"]), gamma=w["g3"], beta=w["be3"], y_out=v(u["x2"]),
               mean=u["mean2"], rstd=u["rstd2"], ff1=dict(K=D, bias=w["b1"], act=o.ACT_RELU), ff2=dict(K=F, bias=w["b2"], self_resid=True),
               proj=head, row_groups=groups)
    dl = u["dlogits"][:M]
    loss = dict(A=v(u["x2"]), B=w["Wo"], labels=w["labels"], loss=u["loss"], T=T, dlogits=dl, probs=u["probs"][:M], logits=u["logits"][:M],
                label_smoothing=ls, downweight=dw, gscale=gscale, M=M, K=D, bias=w["bo"], a_remap=groups, counts=counts)
    dgrad = dict(A=dl, B=w["Wot"], dX_out=v(u["dh"]), x=v(u["h2"]), gamma=w["g3"], mean=u["mean2"], rstd=u["rstd2"], dgamma=None, dbeta=None,
                 mask_mode=2, partials=u["parts3"][:M // 64], M=M, N=D, K=P, c_remap=groups)
    bwd = dict(dff=v(u["dh"]), W2t=w["W2t"], dpre_out=v(u["dpre"]), gate=v(u["a"]), W1t=w["W1t"], dx_out=v(u["dh1"]), x=v(u["h1"]),
               gamma=w["g1"], mean=u["mean1"], rstd=u["rstd1"], dgamma=None, dbeta=None, alpha=1.0, partials=u["parts1"][:M // 64],
               row_groups=groups)
    if fused:
        o.dec_tail_step(fwd, loss, dgrad, bwd)
    else:
        o.ffn_ln_fwd(**fwd)
        kw = {k: x for k, x in loss.items() if k not in ("A", "B", "labels", "loss", "T")}
        o.gemm_sigmoid_bce(loss["A"], loss["B"], loss["labels"], loss["loss"], T, dgrad=dgrad, **kw)
        o.ffn_ln_bwd(**bwd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: L.DT_NAME[d])
def test_dec_tail_step_counts(gpu, dtype):
    from musicstyletransfer_amd import ops as o
    B, T = 2, 64
    assert o.can_dec_tail(D, F, P, T)
    w = _inputs(gpu, B, T, dtype)
    gscale = 1024.0 if dtype == torch.float16 else 4.0
    plain, one, three = (_outputs(gpu, B, T, dtype) for _ in range(3))
    c_one, c_three = Counts(gpu), Counts(gpu)
    _run_tail(o, w, plain, B, T, 0.1, True, gscale, True, None)
    _run_tail(o, w, one, B, T, 0.1, True, gscale, True, c_one.t)
    _run_tail(o, w, three, B, T, 0.1, True, gscale, False, c_three.t)
    got, ref3 = c_one.read("dec_tail_step"), c_three.read("three launches")
    want = roll_ref(three["logits"][:B * T].cpu(), w["labels"].cpu(), P)
    print(f"\ndec_tail_step {L.DT_NAME[dtype]}: counts {got.sum(0).tolist()}, three launches {ref3.sum(0).tolist()}, numpy {want.tolist()}")
    assert np.array_equal(got.sum(0), ref3.sum(0)) and np.array_equal(got.sum(0), want)
    assert 0 < want[0] < want[1] < want[3] == B * T * P and want[2] == int(w["labels"].sum())
    assert not got[B * T // 64:].any() and (got[:B * T // 64, 3] == 64 * P).all()
    for name in list(OUT) + ["loss"]:   # (one 64-row tile per sample: the loss is a single atomic)
        a, b = plain[name].contiguous().view(torch.uint8), one[name].contiguous().view(torch.uint8)
        assert torch.equal(a, b), f"{name} differs from the one-launch run without counts"
    assert not one["dh1"][:-1].view(B, T + 1, -1)[:, 1:].isnan().any() and not one["logits"][:-1].isnan().any()


# ------------------------------------------------------------------------------------------ trainer level
def test_trainer_reports_precision_recall_f1(gpu, tmp_path, monkeypatch):
    """a small piano-roll trainer, dropout 0, four validation steps: pos and cells exactly; pred and tp between the host's counts of
    stored probabilities > 0.5 and >= 0.5 (a stored probability above 0.5 implies a positive logit, and a positive logit implies
    p >= 0.5 in bce_fast and bce_exact alike: a derived bound, not a measured one)"""
    from music_style_transfer.VarAutoEncoder import model, trainer
    from music_style_transfer.VarAutoEncoder.transformer import TransformerConfig
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    from musicstyletransfer_amd.pianoroll import SyntheticPianoRollDataset
    logdir = tmp_path / "tb"
    monkeypatch.setenv("MST_LOGDIR", str(logdir))
    cfg = model.ModelConfig(
        model.EncoderConfig(TransformerConfig(64, 0.0, 2, 2, 128), 16, 2, 128),
        model.DecoderConfig(TransformerConfig(32, 0.0, 1, 2, 128), 16, 2, 128), kind="pianoroll")
    tc = trainer.TrainConfig(batch_size=8, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                             optimizer=trainer.OptimizerConfig("adam", "clip_gradient:1.0", 1e-3), kl_loss=1.0,
                             label_smoothing=0.0, negative_label_downscaling=False, verbose=False, max_steps=9)
    t = trainer.Trainer(tc, gpu_ctx(0), model.Model(cfg), None)

    class Fixed:
        def __init__(self, batches):
            self.batches, self.batch_size = batches, 8

        def __iter__(self):
            return iter(self.batches)

        def num_classes(self):
            return 2

    batches = list(SyntheticPianoRollDataset(8, 32, 32, n_pitches=128, density=0.05, seed=3))[:4]
    assert len(batches) == 4
    t._step(batches[0])                      # one training step first: its counts are cleared with the reset below
    t.collect_metrics(reset=True)
    pos = cells = n_gt = n_ge = tp_gt = tp_ge = 0
    for b in batches:
        t._step(b, is_train=False)
        B, T = b.data[0].shape[:2]
        plan = t._plan(B, T)
        assert plan.track_roll_metrics and plan.cfg.kind == "pianoroll"
        with torch.cuda.stream(t.stream):
            # the same forward pass once more with the eps the step drew, probabilities written out, nothing counted
            probs = torch.zeros(B * T, plan.cfg.out_dim, dtype=plan.adt, device=plan.dev)
            plan.probs, plan.internal_eps, plan.track_roll_metrics = probs, False, False
            plan.forward()
            plan.losses(with_grad=False, combine=False)
            p = probs.float().cpu().numpy().reshape(B, T, -1)
            plan.probs, plan.internal_eps, plan.track_roll_metrics = None, True, True
        lab = np.asarray(b.label[0]) == 1
        pos, cells = pos + int(lab.sum()), cells + lab.size
        n_gt, n_ge = n_gt + int((p > 0.5).sum()), n_ge + int((p >= 0.5).sum())
        tp_gt, tp_ge = tp_gt + int(((p > 0.5) & lab).sum()), tp_ge + int(((p >= 0.5) & lab).sum())
    with torch.cuda.stream(t.stream):
        m = t.model.store.read_metrics(reset=False)
    print(f"\ntrainer: device {[m[k] for k in ('roll_tp', 'roll_pred', 'roll_pos', 'roll_cells')]}; host pos {pos}, cells {cells}, "
          f"pred in [{n_gt}, {n_ge}], tp in [{tp_gt}, {tp_ge}]")
    assert all(isinstance(m[k], int) for k in ("roll_tp", "roll_pred", "roll_pos", "roll_cells"))
    assert m["roll_pos"] == pos and m["roll_cells"] == cells == 4 * 8 * 32 * 128
    assert n_gt <= m["roll_pred"] <= n_ge and tp_gt <= m["roll_tp"] <= tp_ge
    got = t.collect_metrics(reset=True)
    from musicstyletransfer_amd.engine import roll_scores
    assert {k: got[k] for k in ("precision", "recall", "f1", "cell_acc")} == roll_scores(m["roll_tp"], m["roll_pred"], m["roll_pos"], cells)
    assert all(0.0 <= got[k] <= 1.0 for k in ("precision", "recall", "f1", "cell_acc")), got
    after = t.collect_metrics(reset=True)     # right after a reset: nothing counted
    assert all(math.isnan(after[k]) for k in ("precision", "recall", "f1", "cell_acc")), after
    with torch.cuda.stream(t.stream):
        assert t.model.store.read_metrics(reset=False)["roll_cells"] == 0
    # the validation pass of a checkpoint and the scalar log carry the four scores
    t._checkpoint(str(tmp_path / "m"), Fixed(batches))
    assert all(0.0 <= t.last_validation[k] <= 1.0 for k in ("precision", "recall", "f1", "cell_acc")), t.last_validation
    assert "total_loss" in t.last_validation
    t._step(batches[0])
    t._periodic_log(0, 0.0)
    tags = {json.loads(line)["tag"] for line in open(logdir / "scalars.jsonl")}
    assert {"precision", "recall", "f1", "cell_acc", "kl_loss", "total_loss"} <= tags
