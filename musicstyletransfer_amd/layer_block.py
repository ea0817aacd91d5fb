"""The row-wise block of a transformer layer behind the attention mix (W_proj, LayerNorm-1, feed-forward, LayerNorm-2/3) forward and
backward in every launch form, on all rows or on position 0 alone; its weight-gradient problems; the start-up check of the
one-launch position-0 tails. Works on the LayerParams records of params.ParamStore.layer()."""
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import ops as o


class _Layer:
    pass


# Which rows of a layer's [M, ld] buffers a row-wise block works on. view(buf): the operand a launch reads, or a LayerNorm writes; a
# GEMM writes the whole buffer through the output row remap c_remap; ln: the row arguments of the LayerNorm launches.
Rows = namedtuple("Rows", "view c_remap ln")
ALL_ROWS = Rows(lambda buf: buf, (0, 0, 0), {})


def position0_rows(B, S):
    """position 0 of every sample of a [B * S, ld] buffer: B rows, logical row b -> physical row b * S"""
    return Rows(lambda buf: buf.view(B, S, -1)[:, 0, :], (1, S, 0), dict(M=B, row_id_stride=S))


class Dropout(namedtuple("Dropout", "p seed_ptr site0")):
    """dropout of a layer's row-wise block: probability, the device seed word (None at p = 0), the first of the block's three site ids
    (attention output, FFN hidden, FFN output)"""

    def at(self, k):
        """gemm_nt / layernorm_bwd keywords of site k of the block"""
        return dict(dropout_p=self.p, dropout_site=self.site0 + k, dropout_seed_ptr=self.seed_ptr) if self.p > 0 else {}


NO_DROPOUT = Dropout(0.0, None, 0)


def row_block_fwd(P, L, x_in, rows, drop, form, row_groups=None, tail=None, launch=True):
    """The row-wise block of a transformer layer behind the attention mix: W_proj + residual -> LayerNorm-1 -> FF1 + ReLU -> FF2 +
    residual -> LayerNorm-2/3, on `rows` of the layer's buffers L (att in; h1, x1, a, h2, x2, mean1/2, rstd1/2 out). form:
      'launches'  the five launches (any rows: the recovery path of the position-0 tail, and every width without a fused kernel)
      'fused'     one launch, mst_proj_ffn_ln_fwd (all rows; row_groups: ops.ffn_ln_fwd's, the last decoder layer without position 0)
      'tail'      one launch, mst_row_tail_fwd (position-0 rows; tail: its sync / stat_stride / phys_stride / status / rider / queue /
                  shadows keywords)
    launch=False ('fused' only): nothing is launched; returns ops.ffn_ln_fwd's keyword arguments (StepPlan.losses: ops.dec_tail_step)"""
    D, v = P.proj.w.shape[0], rows.view
    if form == "tail":
        o.row_tail_fwd(v(L.att), v(x_in), P.proj.w, P.proj.b, P.ln1.gamma, P.ln1.beta, P.ff1.w, P.ff1.b, P.ff2.w, P.ff2.b, P.ln2.gamma,
                       P.ln2.beta, v(L.h1), v(L.x1), v(L.a), v(L.h2), v(L.x2), L.mean1, L.rstd1, L.mean2, L.rstd2, dropout_p=drop.p,
                       dropout_seed_ptr=drop.seed_ptr, site0=drop.site0, **tail)
        return L.x2
    proj = dict(N=D, K=D, bias=P.proj.b, resid=v(x_in), **drop.at(0))
    ff1 = dict(K=D, bias=P.ff1.b, act=o.ACT_RELU, **drop.at(1))
    ff2 = dict(K=4 * D, bias=P.ff2.b, **drop.at(2))
    ff2.update(dict(self_resid=True) if P.self_resid else dict(resid=v(L.x1)))
    if form == "fused":  # (same results as the five launches, bit for bit in a / h2. The projection's dgrad behind the backward block
        # measured +14 us and was removed.)
        head = dict(att=L.att, W=P.proj.w, h1=L.h1, gamma=P.ln1.gamma, beta=P.ln1.beta, mean=L.mean1, rstd=L.rstd1, **proj)
        kw = dict(x=L.x1, W1=P.ff1.w, a_out=L.a, W2=P.ff2.w, h_out=L.h2, gamma=P.ln2.gamma, beta=P.ln2.beta, y_out=L.x2, mean=L.mean2,
                  rstd=L.rstd2, ff1=ff1, ff2=ff2, proj=head, row_groups=row_groups)
        if not launch:
            return kw
        o.ffn_ln_fwd(**kw)
        return L.x2
    # (Dense + LayerNorm in one launch, ops.gemm_nt_ln_fwd, does not pay in the forward pass: graph-replay timings at
    # M = 16384 are 17.8 vs 19.9 us for N 256 K 256 but 30.3 vs 30.2 for K 1024 and 16.6 vs 13.0 / 21.3 vs 16.5 for
    # N 128, and nothing at step level — the forward LayerNorm is a 7 us launch and the full-row tile costs the GEMM
    # as much. The backward forms, where the LayerNorm launch is 16 us, do pay: row_block_bwd.)
    o.gemm_nt(v(L.att), P.proj.w, L.h1, c_remap=rows.c_remap, **proj)
    o.layernorm_fwd(v(L.h1), P.ln1.gamma, P.ln1.beta, v(L.x1), L.mean1, L.rstd1, D=D, **rows.ln)
    o.gemm_nt(v(L.x1), P.ff1.w, L.a, c_remap=rows.c_remap, **ff1)
    o.gemm_nt(v(L.a), P.ff2.w, L.h2, c_remap=rows.c_remap, **ff2)
    o.layernorm_fwd(v(L.h2), P.ln2.gamma, P.ln2.beta, v(L.x2), L.mean2, L.rstd2, D=D, **rows.ln)
    return L.x2


def _lead_mask(P, t, drop):
    """mask keywords of the LayerNorm backward a layer's backward pass starts with (LN2 of an encoder layer, LN3 of a decoder layer)"""
    if P.mask_mode == 2:
        return dict(mask_mode=2, **drop.at(2))
    return dict(mask_mode=1, dx_masked=t.dhm, **drop.at(2)) if drop.p > 0 else {}


def no_partials(norm, parts):
    """row_block_bwd's `partials` for a block of few rows: the LayerNorm parameter gradients go straight into the bucket (atomics)"""
    return None


def ffn_bwd_parts(L, row_groups=None):
    """workgroups (rows of LayerNorm-1 partials) of a layer's one-launch backward block"""
    M = L.h1.shape[0]
    return o.gemm_nt_ln_parts(M if row_groups is None else M // row_groups[1] * row_groups[0])


def ffn_bwd_kw(P, L, t, drop, partials_buf, row_groups=None):
    """ops.ffn_ln_bwd's keyword arguments (all but lead=) for a layer's one-launch backward block: row_block_bwd 'fused', and
    StepPlan.losses where the block is a phase of ops.dec_tail_step. partials_buf: LayerNorm-1's partials buffer, or None (atomics)."""
    dff = t.dhm if (drop.p > 0 and not P.self_resid) else t.dh
    ln1 = dict(dx_masked=t.dh1m, mask_mode=1, **drop.at(0)) if drop.p > 0 else {}
    return dict(dff=dff, W2t=P.ff2.t, dpre_out=t.dpre, gate=L.a, W1t=P.ff1.t, dx_out=t.dh1, x=L.h1, gamma=P.ln1.gamma, mean=L.mean1,
                rstd=L.rstd1, dgamma=P.ln1.dgamma, dbeta=P.ln1.dbeta, alpha=1.0 / (1.0 - drop.p) if drop.p > 0 else 1.0,
                resid=None if P.self_resid else t.dh, partials=partials_buf, row_groups=row_groups, **ln1)


def row_block_bwd(P, L, t, dy, rows, drop, form, partials, dy_done=False, row_groups=None, tail=None, launch=True, proj_dgrad=True,
                  head=None):
    """Backward of row_block_fwd on the same rows: LayerNorm-2/3 backward of dy, both FFN dgrads, LayerNorm-1 backward, the W_proj
    dgrad. t: the layer's backward buffers — dh, dhm, dx1, dh1m, dpre indexed by the block's own rows, dh1 and datt by the layer's
    (written through `rows`). partials(norm, n_workgroups) -> the partials buffer of one LayerNorm-backward launch, or None
    (StepPlan._ln_partials). Returns (dff, dproj): the A operands of the FF2 and W_proj weight gradients. form:
      'launches'  five launches
      'ln_fused'  FF1 dgrad + LayerNorm-1 backward in one launch (mst_gemm_nt_ln; the gradient in between is never stored): four
      'fused'     both dgrads + LayerNorm-1 backward in one launch (mst_ffn_ln_bwd); an encoder layer's LayerNorm-2 backward rides in
                  its prologue (mst_ffn_ln_bwd_lead; the prologue has no mask_mode 2). row_groups as in row_block_fwd
      'tail'      one launch, mst_row_tail_bwd (position-0 rows; tail: its keywords)
    dy_done: the producer of dy already ran the leading LayerNorm backward (t.dh / t.dhm are filled; not with 'tail').
    launch=False ('fused' with dy_done only): the one-launch block itself is not issued — it ran as a phase of ops.dec_tail_step, from
    ffn_bwd_kw's arguments —; the partial-sum job is registered and the W_proj dgrad issued as always.
    proj_dgrad=False (not with 'tail'): the W_proj dgrad is left to the caller's attention-backward launch (ops.attn_proj_bwd on dproj);
    t.datt is not written.
    head ('fused' with the leading LayerNorm backward in its prologue only; dy is then not read): dict(A, B, resid) — dy = A B^T + resid,
    the K | Q | V input gradient of the layer above, is formed by the one launch itself (ops.ffn_ln_bwd head=)."""
    D, v = P.proj.w.shape[0], rows.view
    if form == "tail":
        o.row_tail_bwd(v(dy), v(L.h2), v(L.h1), v(L.a), L.mean1, L.rstd1, L.mean2, L.rstd2, P.ln1.gamma, P.ln2.gamma, P.ff2.t, P.ff1.t,
                       P.proj.t, t.dh, t.dhm, t.dx1, t.dh1m, t.dpre, v(t.dh1), v(t.datt), P.ln1.dgamma, P.ln1.dbeta, P.ln2.dgamma,
                       P.ln2.dbeta, dropout_p=drop.p, dropout_seed_ptr=drop.seed_ptr, site0=drop.site0, **tail)
        return t.dhm, t.dh1m  # (the launch writes the masked copies at p = 0 too)
    M = L.h1.shape[0]
    lead = None
    if not dy_done and form == "fused" and P.mask_mode == 1:
        lead = dict(dy=None if head is not None else dy, x=L.h2, gamma=P.ln2.gamma, mean=L.mean2, rstd=L.rstd2, dx=t.dh,
                    dgamma=P.ln2.dgamma, dbeta=P.ln2.dbeta,
                    partials=partials(P.ln2, o.gemm_nt_ln_parts(M)), **_lead_mask(P, t, drop))
    elif not dy_done:
        mask = _lead_mask(P, t, drop)
        if P.mask_mode == 2:
            mask["dropout_site"] = drop.site0 + 2  # (this launch has always been given the site id at p = 0 too, where nothing reads it)
        o.layernorm_bwd(v(L.h2), P.ln2.gamma, L.mean2, L.rstd2, v(dy), t.dh, P.ln2.dgamma, P.ln2.dbeta, D=D,
                        partials=partials(P.ln2, o.layernorm_bwd_parts(M, D)), **rows.ln, **mask)
    # encoder: dx feeds the residual branch, its masked copy the feed-forward branch; decoder: one branch (mask_mode 2)
    dff = t.dhm if (drop.p > 0 and not P.self_resid) else t.dh
    resid_ff = None if P.self_resid else t.dh
    # FFN: d(pre-relu) = (dff W2) * 1[a > 0] / (1-p)   (a is stored post-dropout, so a > 0 <=> relu on and kept)
    inv_keep = 1.0 / (1.0 - drop.p) if drop.p > 0 else 1.0
    ln1 = dict(dx_masked=t.dh1m, mask_mode=1, **drop.at(0)) if drop.p > 0 else {}
    if form == "fused":
        buf = partials(P.ln1, ffn_bwd_parts(L, row_groups))
        if head is not None and (lead is None or not launch):
            raise ValueError("row_block_bwd(head=) needs the one launch that starts with the leading LayerNorm backward")
        if launch:
            o.ffn_ln_bwd(lead=lead, head=head, **ffn_bwd_kw(P, L, t, drop, buf, row_groups))
        elif lead is not None:
            raise ValueError("row_block_bwd(launch=False) needs dy_done: the block that ran elsewhere has no leading LayerNorm backward")
    else:
        o.gemm_nt(dff, P.ff2.t, t.dpre, N=4 * D, K=D, gate=v(L.a), alpha=inv_keep)
        if form == "ln_fused":
            o.gemm_nt_ln_bwd(t.dpre, P.ff1.t, t.dh1, L.h1, P.ln1.gamma, L.mean1, L.rstd1, P.ln1.dgamma, P.ln1.dbeta, N=D, K=4 * D,
                             resid=resid_ff, partials=partials(P.ln1, o.gemm_nt_ln_parts(M)), **ln1)
        else:
            o.gemm_nt(t.dpre, P.ff1.t, t.dx1, N=D, K=4 * D, resid=resid_ff)
            o.layernorm_bwd(v(L.h1), P.ln1.gamma, L.mean1, L.rstd1, t.dx1, v(t.dh1), P.ln1.dgamma, P.ln1.dbeta, D=D,
                            partials=partials(P.ln1, o.layernorm_bwd_parts(M, D)), **rows.ln, **ln1)
    dproj = t.dh1m if drop.p > 0 else v(t.dh1)
    if proj_dgrad:
        o.gemm_nt(dproj, P.proj.t, t.datt, N=D, K=D, c_remap=rows.c_remap)
    return dff, dproj


def layer_wgrads(P, L, t, x_in, dff, dproj, rows):
    """a layer's four weight-gradient problems (FF2, FF1, W_proj on `rows`; K | Q | V on every row), for the step's ONE wgrad launch"""
    D, v = P.proj.w.shape[0], rows.view
    return [o.wgrad_problem(dff, v(L.a), P.ff2.dw, P.ff2.db, N=D, K=4 * D),
            o.wgrad_problem(t.dpre, v(L.x1), P.ff1.dw, P.ff1.db, N=4 * D, K=D),
            o.wgrad_problem(dproj, v(L.att), P.proj.dw, P.proj.db, N=D, K=D),
            o.wgrad_problem(t.dqkv, x_in, P.kqv.dw, P.kqv.db, N=3 * D, K=D)]


def row_tail_selfcheck(store, B=64, S=2):
    """One-time start-up check of the one-launch position-0 tails (mst_row_tail_fwd / _bwd) on THIS device, process and
    partition mode: both are run against the five launches the engine falls back to — row_block_fwd / row_block_bwd in both forms —
    on random rows and the store's own top-layer weights. Their grid barrier rests on properties no API guarantees (enough workgroups
    of an oversubscribed launch landing on one XCD, L1 behaviour of write-through lines — csrc/row_tail.hpp), so shape alone does not
    decide whether the fused form is used: a mismatch, an unfinished barrier or a status flag pins the store to the five-launch form."""
    store.tail_checked = True
    cfg, dev, adt = store.cfg, store.device, store.act_dtype
    D, F = cfg.e_model, 4 * cfg.e_model
    if not (o.can_row_tail(B, D) and store.tail_fused and cfg.e_layers >= 1):
        return True
    f32 = dict(dtype=torch.float32, device=dev)
    P = store.layer("encoder", cfg.e_layers - 1)
    # (the check's LayerNorm parameter gradients go to scratch, not into the store's bucket)
    scratch = lambda n: n._replace(dgamma=torch.zeros(D, **f32), dbeta=torch.zeros(D, **f32))
    P = P._replace(ln1=scratch(P.ln1), ln2=scratch(P.ln2))

    def rnd(n, width, site):
        a = torch.zeros(n, width, **f32)
        o.randn(a, seed=0x7A11, site=site)
        t = torch.zeros(n, width, dtype=adt, device=dev)
        o.cast_to_act(a, t)  # (values ~ N(0, 1): LayerNorm makes the chain scale-free)
        return t

    z = lambda n, w: torch.zeros(n, w, dtype=adt, device=dev)
    att, xin = rnd(B * S, D, 1), rnd(B * S, D, 2)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    sync = torch.zeros(8, dtype=torch.int32, device=dev)
    rows = position0_rows(B, S)

    def fbufs():
        L = _Layer()
        L.att, L.h1, L.x1, L.a, L.h2, L.x2 = att, z(B * S, D), z(B * S, D), z(B * S, F), z(B * S, D), z(B * S, D)
        L.mean1, L.rstd1, L.mean2, L.rstd2 = (torch.zeros(B * S, **f32) for _ in range(4))
        return L

    u, f = fbufs(), fbufs()
    tail = dict(stat_stride=S, phys_stride=S, status=status[0:1])
    row_block_fwd(P, u, xin, rows, NO_DROPOUT, "launches")
    row_block_fwd(P, f, xin, rows, NO_DROPOUT, "tail", tail=dict(tail, sync=sync[0:3]))
    # backward chain on the forward's own activations
    dy = rnd(B * S, D, 3)

    def bbufs():
        t = _Layer()
        t.dh, t.dhm, t.dx1, t.dh1m, t.dpre, t.dh1, t.datt = z(B, D), z(B, D), z(B, D), z(B, D), z(B, F), z(B * S, D), z(B * S, D)
        return t

    ub, fb = bbufs(), bbufs()
    row_block_bwd(P, u, ub, dy, rows, NO_DROPOUT, "launches", no_partials)
    row_block_bwd(P, u, fb, dy, rows, NO_DROPOUT, "tail", no_partials, tail=dict(tail, sync=sync[4:7]))
    torch.cuda.current_stream().synchronize()
    want_f, want_b = o.row_tail_barriers(D)
    sy, stv = sync.cpu().tolist(), status.cpu().tolist()
    why = []
    if stv[0]:
        why.append(f"status flags {stv[0]:#x}")
    if sy[0] != want_f or sy[4] != want_b:
        why.append(f"barrier counters {sy[0]} / {sy[4]} instead of {want_f} / {want_b}")
    ulp = 2.0 ** -7 if adt == torch.bfloat16 else 2.0 ** -10
    host = lambda t: t.float().cpu().numpy()
    for k in ("h1", "x1", "a", "h2", "x2"):
        a, b = host(rows.view(getattr(f, k))), host(rows.view(getattr(u, k)))
        if not np.all(np.abs(a - b) <= 4 * ulp * np.maximum(np.abs(b), 1.0)):
            why.append(f"forward {k}: max difference {np.abs(a - b).max():.3g}")
    for k in ("dh", "dpre", "dx1", "dh1", "datt"):
        a, b = host(getattr(fb, k)), host(getattr(ub, k))
        if not np.abs(a - b).max() <= 4 * ulp * max(float(np.abs(b).max()), 1e-6) + 1e-6:
            why.append(f"backward {k}: max difference {np.abs(a - b).max():.3g} (scale {np.abs(b).max():.3g})")
    if why:
        store.tail_fused = False
        warnings.warn("the one-launch position-0 tail failed its start-up check on this device (" + "; ".join(why) +
                      "): using the five-launch form", RuntimeWarning)
    return not why
