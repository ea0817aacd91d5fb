"""Every launch form of the loss heads on a real MI355X against the fp64 references of tests/loss_refs.py: mst_sigmoid_bce (8- and
4-wide sweeps, every label load, both positive counts, one and two workgroups per sample, the decoder's call), mst_gemm_sigmoid_bce
(both tile widths, two column tiles on one atomic, forward only, without probabilities) and _dgrad_ln (one launch and two), mst_softmax_ce
(pad columns, the grid-stride loop, token metrics with planted ties) and the two losses on probabilities — bf16 and fp16, on unit-scale
logits, on saturated ones (`sat`, `wide`) and on logits whose results are known in closed form. Every element inside the derived
bound, every byte outside the results untouched, every launch bit-identical when repeated (the atomically summed losses apart)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_refs as L  # noqa: E402

pytestmark = pytest.mark.gpu
S = L.SENTINEL
BCE_RUNS = [(c, d, m) for c in L.BCE_CASES for d in L.DTYPES for m in c.modes]
FUSED_RUNS = [(c, d, m) for c in L.FUSED_CASES for d in L.DTYPES for m in c.modes]
CE_RUNS = [(c, d, m) for c in L.CE_CASES for d in L.DTYPES for m in c.modes]
_id = lambda r: f"{r[0].id}-{L.DT_NAME[r[1]]}-{r[2]}"  # noqa: E731


def _check(what, name, got, ref, bound, exact=False):
    """every element of got within bound of ref (exact: equal); -> worst error / bound. Failures as the attention suite reports them"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    bound = np.broadcast_to(np.atleast_2d(bound), got.shape)
    assert np.isfinite(got).all(), f"{what}: {name} holds a non-finite value"
    err = np.abs(got - ref)
    bad = (got != ref) if exact else ~(err <= bound)
    ratio = err / np.maximum(bound, 1e-300)
    if bad.any():
        g2, r2, b2, bad2, ratio2 = (x.reshape(-1, x.shape[-1]) for x in (got, ref, bound, bad, ratio))
        i, j = np.unravel_index(np.argmax(np.where(bad2, np.maximum(ratio2, 1e-300), 0)), bad2.shape)
        rows, cols = np.nonzero(bad2)
        pytest.fail(f"{what}: {int(bad.sum())}/{bad.size} elements of {name} outside the bound; worst at row {i}, column {j} of "
                    f"{g2.shape}: got {g2[i, j]!r}, want {r2[i, j]!r}, bound {b2[i, j]:.3g}; rows {rows.min()}..{rows.max()}, columns "
                    f"{cols.min()}..{cols.max()}, {len(np.unique(rows))} rows, {len(np.unique(cols))} columns")
    return 0.0 if exact else float(ratio.max())


class Guarded:
    """an output of `rows` x `width` at leading dimension ld, `off` elements into a sentinel-filled allocation with two rows more behind
    it: .t is what the launch is given, .intact(rows, width) says that nothing but the result (and `zeroed` pad columns) was written"""

    def __init__(self, rows, ld, dtype, gpu, off=0, fill=S):
        self.off, self.rows, self.ld = off, rows, ld
        self.flat = torch.full((off + (rows + 2) * ld + 8,), fill, dtype=dtype, device=gpu)
        self.t = self.flat[off:off + (rows + 2) * ld].view(rows + 2, ld)
        self.fill = fill

    def host(self):
        self.h = self.flat.cpu()
        return self.h[self.off:self.off + (self.rows + 2) * self.ld].view(self.rows + 2, self.ld)

    def intact(self, width, zero_to=None, rows=None):
        """after host(): the columns [width, ld) of the result rows (those up to zero_to: zero), the rows behind, and both ends"""
        v = self.h[self.off:self.off + (self.rows + 2) * self.ld].view(self.rows + 2, self.ld)
        n = self.rows if rows is None else rows
        zero_to = width if zero_to is None else zero_to
        ok = (self.h[:self.off] == self.fill).all() and (self.h[self.off + (self.rows + 2) * self.ld:] == self.fill).all()
        ok = ok and (v[n:] == self.fill).all() and (v[:n, zero_to:] == self.fill).all() and (v[:n, width:zero_to] == 0).all()
        return bool(ok)


def _same_bits(a, b):
    return torch.equal(a.flat.view(torch.uint8), b.flat.view(torch.uint8))


def _nonzero_where_representable(what, got, ref, bound):
    """fp16 gradients the bound says are representable did not underflow"""
    must = np.abs(ref) > bound
    assert (got[must] != 0).all(), f"{what}: {int((got[must] == 0).sum())} gradients that are representable came out zero"


# ------------------------------------------------------------------------------------------ mst_sigmoid_bce
def _run_bce(o, c, dev, dtype, gpu):
    M = c.B * c.T
    probs = Guarded(M, c.ldp, dtype, gpu, c.off_p)
    dl = None if c.decoder else Guarded(M, c.ldd, dtype, gpu, c.off_d)
    # pre_zeroed = 0 must overwrite whatever loss holds; pre_zeroed = 1 (the decoder's call) adds to zeros
    loss = Guarded(1, c.B, torch.float32, gpu)
    if c.decoder:
        loss.t[0].zero_()
    npos = torch.full((c.B + 2,), -7, dtype=torch.int32, device=gpu)
    o.sigmoid_bce(dev["logits"], dev["labels"], loss.t[0], c.B, c.T, c.P, label_smoothing=c.ls, downweight=c.dw, npos=npos, probs=probs.t,
                  dlogits=None if dl is None else dl.t, gscale=c.gscale, pre_zeroed=c.decoder)
    torch.cuda.synchronize()
    return dict(probs=probs, dlogits=dl, loss=loss, npos=npos)


@pytest.mark.parametrize("run", BCE_RUNS, ids=_id)
def test_sigmoid_bce_form_against_fp64(gpu, run):
    from musicstyletransfer_amd import ops as o
    c, dtype, mode = run
    what = f"sigmoid_bce {c.id} {L.DT_NAME[dtype]} {mode}"
    host = L.bce_operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    assert dev["labels"].data_ptr() % 8 == 0
    got, again = _run_bce(o, c, dev, dtype, gpu), _run_bce(o, c, dev, dtype, gpu)
    f = L.form_tuple(o.sigmoid_bce_form(dtype, c.B, c.T, c.P, dev["logits"], c.ld, dev["labels"], c.ls, c.dw, got["npos"], got["loss"].t,
                                        got["probs"].t, c.ldp, None if c.decoder else got["dlogits"].t, c.ldd, c.gscale, c.decoder))
    assert f == c.form, f"{what}: the launch takes {f}, the case is meant for {c.form}"
    for k in ("probs", "dlogits") + (("loss",) if f[4] == 1 else ()):
        assert got[k] is None or _same_bits(got[k], again[k]), f"{what}: {k} differs between two launches"
    assert torch.equal(got["npos"], again["npos"])

    r = L.bce_references(c.id, dtype, mode)
    M, P, Pz = c.B * c.T, c.P, L.roundup(c.P, 4)
    worst = {}
    known = L.bce_known(host["labels"].numpy().reshape(c.B, c.T, P), c.ls, c.dw, c.gscale, c.T, P, dtype) if mode == "known" else None
    probs = got["probs"].host().double().numpy()[:M, :P]
    worst["probs"] = _check(what, "probs", probs, r["probs"].reshape(M, P), r["b_probs"].reshape(M, P))
    assert got["probs"].intact(P, Pz), f"{what}: a store outside probs (pad columns {P}..{Pz} are written as zeros)"
    if known is not None:
        _check(what, "probs (closed form)", probs, known[0].reshape(M, P), 0.0, exact=True)
    if not c.decoder:
        dl = got["dlogits"].host().double().numpy()[:M, :P]
        ref, bound = r["dlogits"].reshape(M, P), r["b_dlogits"].reshape(M, P)
        worst["dlogits"] = _check(what, "dlogits", dl, ref, bound)
        assert got["dlogits"].intact(P, Pz), f"{what}: a store outside dlogits"
        _nonzero_where_representable(what, dl, ref, bound)
        if known is not None:
            ex = known[2].reshape(M, P)
            _check(what, "dlogits (closed form)", np.where(ex, dl, 0.0), np.where(ex, known[1].reshape(M, P), 0.0), 0.0, exact=True)
    loss = got["loss"].host().double().numpy()[0]
    worst["loss"] = _check(what, "loss", loss, r["loss"], r["b_loss"])
    assert got["loss"].intact(c.B, rows=1), f"{what}: a store behind loss"
    npos = got["npos"].cpu().numpy()
    if c.dw:
        assert np.array_equal(npos[:c.B], r["npos"]), f"{what}: npos {npos[:c.B]}, want {r['npos']}"
    else:
        assert (npos[:c.B] == -7).all(), f"{what}: npos written without down-weighting"
    assert (npos[c.B:] == -7).all()
    print(f"\n{what}: form {f}; worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------ the fused launches
def _run_fused(o, c, dev, dtype, gpu):
    M, P, K, Sd = c.M, c.P, c.K, c.T + 1
    g = lambda rows, ld, dt=dtype: Guarded(rows, ld, dt, gpu)  # noqa: E731
    out = dict(dlogits=g(M, P + 8) if c.with_c else None, probs=g(M, P + 8) if c.with_probs else None, logits=g(M, P + 8),
               loss=Guarded(1, c.B, torch.float32, gpu))
    out["loss"].t[0].zero_()        # "loss[b] must be zero on entry"
    kw = dict(dlogits=None if out["dlogits"] is None else out["dlogits"].t, probs=None if out["probs"] is None else out["probs"].t,
              logits=out["logits"].t, label_smoothing=c.ls, downweight=c.dw, gscale=c.gscale, M=M, K=K, bias=dev["bias"], alpha=c.alpha,
              a_remap=(c.T, Sd, 1))
    dgrad = None
    if c.dgrad:
        parts = o.gemm_nt_ln_parts(M)
        out.update(dx=g(c.B * Sd, K + 8), parts=g(parts, 2 * K, torch.float32), dgamma=g(1, K, torch.float32), dbeta=g(1, K, torch.float32))
        dgrad = dict(A=out["dlogits"].t, B=dev["Wt"], dX_out=out["dx"].t, x=dev["h"], gamma=dev["gamma"], mean=dev["mean"], rstd=dev["rstd"],
                     dgamma=out["dgamma"].t[0], dbeta=out["dbeta"].t[0], mask_mode=2, partials=out["parts"].t[:parts], M=M, N=K, K=P,
                     c_remap=(c.T, Sd, 1))
        if c.drop > 0:
            dgrad.update(dropout_p=c.drop, dropout_seed_ptr=dev["seed"], dropout_site=L.FUSED_SITE)
    o.gemm_sigmoid_bce(dev["x"], dev["W"], dev["labels"], out["loss"].t[0], c.T, dgrad=dgrad, **kw)
    torch.cuda.synchronize()
    return out, kw, dgrad


@pytest.mark.parametrize("run", FUSED_RUNS, ids=_id)
def test_gemm_sigmoid_bce_form_against_fp64(gpu, run):
    from musicstyletransfer_amd import ops as o
    c, dtype, mode = run
    what = f"gemm_sigmoid_bce {c.id} {L.DT_NAME[dtype]} {mode}"
    host = L.fused_operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    dev["seed"] = torch.tensor([L.FUSED_SEED_WORD, 0, 0, 0], dtype=torch.int64, device=gpu)
    (got, kw, dgrad), (again, _, _) = _run_fused(o, c, dev, dtype, gpu), _run_fused(o, c, dev, dtype, gpu)
    g, q = o._gemm_bce_args(dev["x"], dev["W"], dev["labels"], got["loss"].t[0], c.T, **kw)
    g2, l = o._gemm_ln_bwd_args(**dgrad) if dgrad else (None, None)
    f = o.gemm_sigmoid_bce_form(g, q, g2, l)
    f = (f["BN"], f["col_tiles"], f["launches"])
    assert f == c.form, f"{what}: the launch takes {f}, the case is meant for {c.form}"
    one_atomic = c.T == 64 and f[1] == 1      # one workgroup per sample
    for k, v in got.items():
        if v is not None and (k != "loss" or one_atomic):
            assert _same_bits(v, again[k]), f"{what}: {k} differs between two launches"

    M, P, K = c.M, c.P, c.K
    worst = {}
    lg16 = got["logits"].host()[:M, :P]
    ref, bound = L.fused_logits_ref(c, host, dtype)
    worst["logits"] = _check(what, "logits", lg16.double().numpy(), ref, bound, exact=(mode == "known"))
    assert got["logits"].intact(P), f"{what}: a store outside logits"
    # the loss of the logits the launch itself stored: a GEMM result on a rounding boundary is not the loss's mistake
    r = L.bce_reference_on(lg16, host["labels"], c, dtype)
    known = L.bce_known(host["labels"].numpy().reshape(c.B, c.T, P), c.ls, c.dw, c.gscale, c.T, P, dtype) if mode == "known" else None
    if c.with_probs:
        probs = got["probs"].host().double().numpy()[:M, :P]
        worst["probs"] = _check(what, "probs", probs, r["probs"].reshape(M, P), r["b_probs"].reshape(M, P))
        assert got["probs"].intact(P), f"{what}: a store outside probs"
        if known is not None:
            _check(what, "probs (closed form)", probs, known[0].reshape(M, P), 0.0, exact=True)
    if c.with_c:
        dl16 = got["dlogits"].host()[:M, :P]
        dl = dl16.double().numpy()
        ref, bound = r["dlogits"].reshape(M, P), r["b_dlogits"].reshape(M, P)
        worst["dlogits"] = _check(what, "dlogits", dl, ref, bound)
        assert got["dlogits"].intact(P), f"{what}: a store outside dlogits"
        _nonzero_where_representable(what, dl, ref, bound)
        if known is not None:
            ex = known[2].reshape(M, P)
            _check(what, "dlogits (closed form)", np.where(ex, dl, 0.0), np.where(ex, known[1].reshape(M, P), 0.0), 0.0, exact=True)
    loss = got["loss"].host().double().numpy()[0]
    worst["loss"] = _check(what, "loss", loss, r["loss"], r["b_loss"])
    assert got["loss"].intact(c.B, rows=1), f"{what}: a store behind loss"
    if c.dgrad:  # the backward GEMM + LayerNorm backward on the dlogits the launch stored
        d = L.fused_dgrad_ref(c, host, dl16, dtype)
        pm = L.phys_rows(c)
        dxh = got["dx"].host()
        worst["dX"] = _check(what, "dX_out", dxh[torch.from_numpy(pm), :K].double().numpy(), *d["dx"])
        rest = np.setdiff1d(np.arange(dxh.shape[0]), pm)
        assert (dxh[torch.from_numpy(rest)] == S).all() and (dxh[:, K:] == S).all(), f"{what}: a store outside the remapped rows of dX_out"
        parts = o.gemm_nt_ln_parts(M)
        ph = got["parts"].host().double().numpy()
        assert got["parts"].intact(2 * K, rows=parts), f"{what}: a store behind the LayerNorm partials"
        assert np.isfinite(ph[:parts]).all()
        sums = ph[:parts].sum(0)
        worst["dgamma"] = _check(what, "dgamma partials", sums[:K], *d["dgamma"])
        worst["dbeta"] = _check(what, "dbeta partials", sums[K:], *d["dbeta"])
        for k in ("dgamma", "dbeta"):
            got[k].host()
            assert got[k].intact(0, rows=1), f"{what}: {k} touched although the partial rows were asked for"
    print(f"\n{what}: form {f}; worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------ mst_softmax_ce
def _run_ce(o, c, dev, dtype, gpu, tok):
    M = c.M
    probs = Guarded(M, c.ldp or c.V + 3, torch.float32, gpu) if c.with_probs else None
    dl = Guarded(M, c.ldd, dtype, gpu) if c.with_dl else None
    loss = Guarded(1, c.B, torch.float32, gpu)
    if c.decoder:
        loss.t[0].zero_()
    o.softmax_ce(dev["logits"], dev["labels"], loss.t[0], c.B, c.T, c.V, probs=None if probs is None else probs.t,
                 dlogits=None if dl is None else dl.t, gscale=c.gscale, pre_zeroed=c.decoder, tok_parts=tok, top_k=c.top_k)
    torch.cuda.synchronize()
    return dict(probs=probs, dlogits=dl, loss=loss)


@pytest.mark.parametrize("run", CE_RUNS, ids=_id)
def test_softmax_ce_form_against_fp64(gpu, run):
    from musicstyletransfer_amd import ops as o
    c, dtype, mode = run
    what = f"softmax_ce {c.id} {L.DT_NAME[dtype]} {mode}"
    host = L.ce_operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    n_tok = 4 * L.CE_MAX_WORKGROUPS
    tok_flat = torch.full((n_tok + 8,), S, dtype=torch.float32, device=gpu)
    tok = tok_flat[4:4 + n_tok].view(L.CE_MAX_WORKGROUPS, 4)
    tok.zero_()
    got, again = _run_ce(o, c, dev, dtype, gpu, tok), _run_ce(o, c, dev, dtype, gpu, tok)   # tok_parts is added to: twice
    for k in ("probs", "dlogits") + (("loss",) if c.T == 1 else ()):
        assert got[k] is None or _same_bits(got[k], again[k]), f"{what}: {k} differs between two launches"

    r = L.ce_references(c.id, dtype, mode)
    M, V = c.M, c.V
    labels = host["labels"].numpy().astype(np.int64)
    known = L.ce_known(c, labels, dtype) if mode == "known" else None
    worst = {}
    if c.with_probs:
        probs = got["probs"].host().double().numpy()[:M, :V]
        worst["probs"] = _check(what, "probs", probs, r["probs"], r["b_probs"])
        assert got["probs"].intact(V), f"{what}: a store outside probs"
        if known is not None:
            _check(what, "probs (closed form)", probs, known[0], 0.0, exact=True)
    if c.with_dl:
        dl = got["dlogits"].host().double().numpy()[:M, :V]
        worst["dlogits"] = _check(what, "dlogits", dl, r["dlogits"], r["b_dlogits"])
        assert got["dlogits"].intact(V, c.zero_end), f"{what}: pad columns {V}..{c.zero_end} of dlogits not zero, or a store behind them"
        _nonzero_where_representable(what, dl, r["dlogits"], r["b_dlogits"])
        if known is not None:
            _check(what, "dlogits (closed form)", dl, known[1], 0.0, exact=True)
    loss = got["loss"].host().double().numpy()[0]
    worst["loss"] = _check(what, "loss", loss, r["loss"], r["b_loss"])
    assert got["loss"].intact(c.B, rows=1), f"{what}: a store behind loss"
    th = tok_flat.cpu().double().numpy()
    assert (th[:4] == S).all() and (th[4 + n_tok:] == S).all(), f"{what}: a store outside tok_parts"
    rows = th[4:4 + n_tok].reshape(-1, 4)
    assert not rows[c.grid:].any(), f"{what}: a tok_parts row beyond the grid's {c.grid} workgroups was written"
    sums = rows.sum(0)
    assert np.array_equal(sums[1:], 2.0 * r["tok"][1:]), f"{what}: token counts {sums[1:] / 2}, want {r['tok'][1:]} (arg-max, top-{c.top_k}, valid)"
    worst["nll"] = _check(what, "sum -log max(p, 1e-10) of two launches", sums[0], 2.0 * r["tok"][0],
                          2.0 * r["b_nll"] + 4.0 * L.U * abs(r["tok"][0]))
    print(f"\n{what}: grid {c.grid}{', strided' if c.strided else ''}; worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------ the losses on probabilities
@pytest.mark.parametrize("dtype", L.PROB_DTYPES, ids=lambda d: L.DT_NAME[d])
def test_losses_from_probabilities_against_fp64(gpu, dtype):
    from musicstyletransfer_amd import ops as o
    what = f"from_probs {L.DT_NAME[dtype]}"
    host = L.probs_operands(dtype)
    dev = {k: v.to(gpu) for k, v in host.items()}
    B, T, V = L.PROBS_B, L.PROBS_T, L.PROBS_V
    worst = {}

    def twice(fn):
        outs = []
        for _ in range(2):
            loss = Guarded(1, B, torch.float32, gpu)
            fn(loss.t[0])
            torch.cuda.synchronize()
            outs.append(loss)
        assert _same_bits(*outs), f"{what}: the loss differs between two launches: there are no atomics"
        h = outs[0].host().double().numpy()[0]
        assert outs[0].intact(B, rows=1), f"{what}: a store behind loss"
        return h

    ref, bound = L.ce_probs_ref(host["ce_probs"][:, :V].double().numpy(), host["ce_labels"].numpy().astype(np.int64), B, T)
    worst["ce"] = _check(what, "ce_from_probs", twice(lambda loss: o.ce_from_probs(dev["ce_probs"], dev["ce_labels"], loss, B, T, V)), ref, bound)
    for ls in (0.0, 0.1):
        for dw in (False, True):
            ref, bound = L.bce_probs_ref(host["bce_probs"].double().numpy(), host["bce_labels"].numpy(), ls, dw)
            got = twice(lambda loss: o.bce_from_probs(dev["bce_probs"], dev["bce_labels"], loss, label_smoothing=ls, downweight=dw))
            worst[f"bce ls {ls} dw {int(dw)}"] = _check(what, f"bce_from_probs ls {ls} dw {dw}", got, ref, bound)
    print(f"\n{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
