"""Step engine: sequences the C-ABI kernels (include/mst_hip.h) into the VarAutoEncoder training
step of the reference — Trainer._step (VarAutoEncoder/trainer.py:155-179): forward
(model.py:287-296), CE/BCE + beta*KL (loss.py), backward, MXNet-rule Adam — with every
intermediate resident in HBM buffers allocated once, and the whole step captured in a hipGraph.

Layout in HBM
  * ParamStore: ONE flat fp32 buffer each for parameters, gradients (the bucket RCCL all-reduces),
    Adam m and v; a same-offset 16-bit shadow (GEMM B operands) and a second flat buffer of
    transposed 16-bit shadows (dgrad B operands / piano-roll embedding tables). W_k, W_q, W_v of a
    layer sit back to back so the three reference Dense layers run as one [3D, D] GEMM.
  * StepPlan(B, T): activations as [rows, ld] 16-bit matrices (ld = roundup8(width), pad columns
    zero), saved for backward; fp32 only for softmax statistics, LayerNorm mean/rstd, the latent
    block and the losses.

There is no torch autograd, no torch operator and no CPU fallback on this path: backward is written
out by hand below, mirroring the forward line by line.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import ops as o
from ._lib import CE_MAX_WORKGROUPS, ROLL_SLOTS  # noqa: F401  (re-exported)
from .ops import roundup
# the engine's parts, re-exported under the names they have always had here
from .spec import VAEConfig, logical_param_shapes, positional_table, xavier_init  # noqa: F401
from .step_math import (check_class_mmd, check_clip, check_ema, check_input_dropout, check_iw, check_schedule, class_mmd_score,  # noqa: F401
                        clip_scale, ema_decay_at, ema_update, iw_scores, latent_scores, roll_scores, schedule_values)
from .params import Dense, LayerParams, Norm, ParamStore  # noqa: F401
from .layer_block import (ALL_ROWS, NO_DROPOUT, Dropout, Rows, _Layer, _lead_mask, ffn_bwd_kw, ffn_bwd_parts, layer_wgrads,  # noqa: F401
                          no_partials, position0_rows, row_block_bwd, row_block_fwd, row_tail_selfcheck)
from .iw import IWBound  # noqa: F401


# The launch forms of one issued kernel sequence (StepPlan._resolve_forms): tails — the position-0 tails as one launch; riders — GEMMs
# riding on them; shadows — where the transposed-shadow refresh goes ('own' / 'begin' / 'tail'); the rest as named there.
# sched — the latent block's backward launch and the step-closing bookkeeping in their scheduled forms (training schedules on).
# dec_tail — the last decoder layer's row-wise block, the loss launch and the block's backward as ONE launch (a training step with gradient).
# gnorm — the optimizer clips by the global gradient norm: one mst_grad_sumsq launch ahead of the Adam launches in their gnorm form.
# ema — the Adam launches in their averaging form (mst_adam_args.ema): the same launches in the same order, none added.
# attn_proj_e / attn_proj_d — the W_proj input gradient of an encoder layer below the top one / of a (non-causal) decoder layer is formed
# inside its attention-backward launch (mst_attn_proj_bwd) instead of by a GEMM launch that writes datt.
# kqv_head_e — the K | Q | V input gradient of an encoder layer above another one is formed inside that layer's feed-forward backward launch
# (mst_kqv_ffn_ln_bwd), in front of the leading LayerNorm backward, instead of by a GEMM launch that writes the gradient.
Forms = namedtuple("Forms", "tails riders shadows fuse_bce bce_dgrad skip_row0 cls_fold ffn_e ffn_d ln_bwd_e ln_bwd_d sched dec_tail gnorm ema "
                            "attn_proj_e attn_proj_d kqv_head_e in_drop")


class StepPlan:
    """All buffers and the kernel sequence of one training step at a fixed (B, T)."""

    def __init__(self, store, B, T, lr=3e-4, clip_gradient=1.0, kl_weight=1.0, label_smoothing=0.0,
                 negative_label_downscaling=False, global_batch=None, gscale=None, want_probs=False, seed=0,
                 internal_eps=False, optimizer_params=None, sample_offset=0, site_base=0,
                 kl_warmup_steps=0, kl_cycle_steps=0, kl_free_bits=0.0, lr_warmup_steps=0, clip_global_norm=0.0, ema_decay=0.0,
                 d_input_dropout=0.0):
        """kl_warmup_steps / kl_cycle_steps / kl_free_bits / lr_warmup_steps: the training schedules (schedule_values),
        evaluated on the device from Adam's step count. All zero (the default): the plain launches with their constants.
        clip_global_norm: bound on the global L2 norm of the batch-mean gradient, applied on the device ahead of Adam (clip_scale;
        DESIGN §12); a step whose norm is not finite is skipped. 0 (the default): off, the optimizer launches as they were.
        ema_decay: decay of an exponential moving average of the weights kept by the Adam launch(es) themselves in store.ema (ema_decay_at,
        ema_update). 0 (the default): off, the optimizer launches as they were.
        d_input_dropout: probability that a training step hides a decoder input position (the previous frame / token) from the
        teacher-forced decoder, drawn on the device by the step's bookkeeping launch (include/mst_hip.h: mst_step_begin_args.in_*;
        DESIGN §16). 0 (the default): off, the launches as they were. Inference passes and validation steps never drop.
        sample_offset: index of this plan's first sample in the global batch (data parallel: rank * B) — the in-graph eps and the
        decoder-input dropout mask are drawn per GLOBAL sample index, so the result does not depend on the sharding.
        site_base: added to every dropout site id (data parallel: a different value per rank gives every rank its own
        masks under the common step seed)."""
        cfg = store.cfg
        self.store, self.cfg, self.B, self.T = store, cfg, B, T
        self.dev, self.adt = store.device, store.act_dtype
        self.lr, self.clip, self.kl_weight = lr, clip_gradient, kl_weight
        check_schedule(kl_warmup_steps, kl_cycle_steps, kl_free_bits, lr_warmup_steps)
        self.schedule = dict(kl_warmup_steps=int(kl_warmup_steps), kl_cycle_steps=int(kl_cycle_steps), kl_free_bits=float(kl_free_bits),
                             lr_warmup_steps=int(lr_warmup_steps))
        self.scheduled = any(self.schedule.values())  # resolved once: the scheduled launches, or the plain ones
        check_clip(clip_global_norm)
        self.clip_global_norm = float(clip_global_norm)
        self.grad_parts = store.grad_parts() if self.clip_global_norm > 0 else None  # (allocated here, never inside a capture)
        check_ema(ema_decay)
        self.ema_decay = float(ema_decay)
        if self.ema_decay > 0:
            store.enable_ema()  # (a copy of w, made here, never inside a capture)
        check_input_dropout(d_input_dropout)
        self.d_input_dropout = float(d_input_dropout)
        self._infer = self._tick_adam = False  # (set by forward() / the step; _resolve_forms below reads them)
        self.ls, self.nld = label_smoothing, negative_label_downscaling
        self.global_batch = global_batch or B
        self.sample_offset, self.site_base = int(sample_offset), int(site_base)
        if (self.sample_offset * cfg.latent_dim) % 2:
            raise ValueError("sample_offset * latent_dim must be even (eps is drawn in Box-Muller pairs)")
        # fp16 needs loss scaling for the 1/(T*P)-sized reconstruction gradients (decoder side); bf16 does
        # not. The encoder side is fed by the KL term, whose sigma - 1/sigma gradient is huge near sigma = 0
        # (loss.py:9 has no epsilon), so it keeps scale 1: the two halves of the flat bucket carry their own
        # scale and Adam un-scales each range.
        self.gscale = gscale if gscale is not None else (1024.0 if self.adt == torch.float16 else 1.0)
        self.gscale_enc = 1.0
        self.want_probs, self.internal_eps = want_probs, internal_eps
        self.opt = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0)
        if optimizer_params:
            for k_src, k_dst in (("beta1", "beta1"), ("beta2", "beta2"), ("epsilon", "eps"), ("wd", "wd")):
                if k_src in optimizer_params:
                    self.opt[k_dst] = float(optimizer_params[k_src])
        dev, adt = self.dev, self.adt
        De, Dd, Z = cfg.e_model, cfg.d_model, cfg.latent_dim
        Se, Sd = T, T + 1
        self.Me, self.Md = B * Se, B * Sd
        f32 = dict(dtype=torch.float32, device=dev)

        def act(rows, width):
            return torch.zeros(rows, roundup(width, 8), dtype=adt, device=dev)

        # RIDERS on the one-launch position-0 tails (which keep ONE XCD busy for ~26 us each while seven idle): the decoder's first
        # K | Q | V projection of rows 1..T — its input exists since the step's first launch — is computed by the forward tail
        # launch's workgroups on the other XCDs (row 0 by the latent block's launch), and the input gradient of that projection for
        # rows 1..T — which only the decoder embedding's weight gradient reads — by the backward tail's (row 0 inside the latent
        # block's backward launch): two GEMM launches (12 + 10 us at configs[1]) leave the step's dependent chain. Piano-roll ends.
        self.ride = (cfg.kind != "token" and cfg.d_layers >= 1 and cfg.e_layers >= 1 and Dd in (128, 256) and
                     o.can_ride(B * T, 3 * Dd, Dd, T) and o.can_ride(B * T, Dd, 3 * Dd, T))
        # the deferred shadow refresh (ParamStore.shadows_deferred) behind the forward tail's riders where that launch has them;
        # False: behind the tiles of the step's first launch
        self.shadows_on_tail = True
        # the last decoder layer's row-wise block, the loss and the block's backward in one launch where the shape has that form
        # (ops.dec_tail_pays) and the step is a training step; False: the three launches (diagnostics, tests)
        self.dec_tail = True
        # an encoder layer's K | Q | V input gradient inside the feed-forward backward launch of the layer below, where the library takes
        # the shape that way (ops.kqv_head_pays); False: the GEMM launch (diagnostics, tests)
        self.kqv_head = True
        self.n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count if self.dev.type == "cuda" else 0
        # the launch forms of the sequence issued last (resolved again by every forward(); here: the buffers below follow from them)
        self.forms = self._resolve_forms()
        # ---- inputs: ONE static device blob (so a batch arrives with a single copy) viewed as typed tensors
        if cfg.kind == "token":
            seg = [("tokens", B * T * 4), ("labels", B * T * 4)]
        else:
            # piano-roll frames stay uint8 in HBM, exactly as the batcher delivers them (1 byte per pitch; rows padded to 8):
            # the embedding GEMMs and their weight gradients widen them while staging tiles into LDS (a_u8); with Forms.cls_fold
            # the one-hot class id of a frame sits in C extra columns behind its pitches
            self.ld_roll = roundup(cfg.in_dim + (cfg.num_classes if self.forms.cls_fold else 0), 8)
            seg = [("roll", B * T * self.ld_roll), ("labels", B * T * cfg.out_dim)]
        seg += [("seq_lens", B * 4), ("classes", B * 4)]
        self.in_layout, off = {}, 0
        for name, nbytes in seg:
            self.in_layout[name] = (off, nbytes)
            off = roundup(off + nbytes, 16)
        self.own_inbuf = torch.zeros(off, dtype=torch.uint8, device=dev)
        self.bind_inputs(self.own_inbuf)
        # decoder-input dropout (allocated here, never inside a capture): the step's keep mask, one byte per decoder input position, and
        # on the piano-roll ends the frames with the dropped rows zeroed — the A operand of the decoder's embedding GEMM and of its
        # weight gradient in place of `roll` (rows as wide as that view, with a leading dimension of their own)
        self.in_keep = self.roll_d = None
        if self.d_input_dropout > 0:
            self.in_keep = torch.zeros(B * T, dtype=torch.uint8, device=dev)
            if cfg.kind != "token":
                self.roll_d = torch.zeros(B * T, roundup(cfg.in_dim, 8), dtype=torch.uint8, device=dev)
        self.eps = torch.zeros(B, Z, **f32)
        self.rng_state = store.rng_state(seed)
        self._outers = []
        self._cls_job = None

        self.pos_e = torch.from_numpy(positional_table(De, Se)).to(dev)
        self.pos_d = torch.from_numpy(positional_table(Dd, Sd)).to(dev)
        self.keymask_e = torch.zeros(B, Se, dtype=torch.uint8, device=dev)
        self.keymask_d = torch.zeros(B, Sd, dtype=torch.uint8, device=dev)

        def layers(n, M, D, H, S):
            out = []
            for _ in range(n):
                L = _Layer()
                L.qkv, L.att, L.h1, L.x1 = act(M, 3 * D), act(M, D), act(M, D), act(M, D)
                L.a, L.h2, L.x2 = act(M, 4 * D), act(M, D), act(M, D)
                L.lse = torch.zeros(2, B, H, S, **f32)
                L.mean1, L.rstd1 = torch.zeros(M, **f32), torch.zeros(M, **f32)
                L.mean2, L.rstd2 = torch.zeros(M, **f32), torch.zeros(M, **f32)
                out.append(L)
            return out

        self.x0_e = act(self.Me, De)
        self.enc = layers(cfg.e_layers, self.Me, De, cfg.e_heads, Se)
        self.x0_d = act(self.Md, Dd)
        self.dec = layers(cfg.d_layers, self.Md, Dd, cfg.d_heads, Sd)
        self.mu, self.sigma, self.z = torch.zeros(B, Z, **f32), torch.zeros(B, Z, **f32), torch.zeros(B, Z, **f32)
        self.kl, self.total = torch.zeros(B, **f32), torch.zeros(B, **f32)
        # per-sample reconstruction sums: accumulated with atomics, cleared by the step's first launch (size padded to 16 B);
        # the same zero list clears the grid-barrier words of the one-launch position-0 tails (mst_row_tail_*)
        nb4 = (B + 3) // 4 * 4
        # (+ 8 sync words of the position-0 tail launches, zeroed with it by step_begin; + the two tile queues of the tails' riders,
        # each in a 128-byte line of its own: next to the barrier words their ticket atomics delayed the chain's barriers)
        self._recon_buf = torch.zeros(nb4 + 8 + 24 + 64, **f32)
        self.recon = self._recon_buf[:B]
        self.sync_words = self._recon_buf[nb4: nb4 + 8].view(torch.int32)
        self.ride_queues = self._recon_buf[nb4 + 32:].view(torch.int32)  # [0]: forward tail's riders, [32]: backward tail's
        self.metric_acc = store.metric_acc  # [sum kl, sum total, count]  (trainer.py:115-116)
        self.track_token_metrics = False  # Trainer: accumulate ppl / acc / topk sums on the device in the CE launch
        self.track_roll_metrics = False   # Trainer: count tp / pred / pos / cells on the device in whichever launch computes the BCE
        # Trainer: one launch behind the latent block's adds the batch's per-class, per-dimension sums of mu, mu^2, sigma^2 and kl_d to
        # store.lat_stats (training steps and validation forwards, never inference; not undone by the step guards, as roll_counts)
        self.track_latent_stats = False
        # Trainer: the class-conditional MMD penalty on z, lambda and the kernel's bandwidth s2 (None: the latent width Z). With
        # lambda > 0 a training step issues mst_class_mmd directly behind the latent block's backward launch, with the gradient pointers;
        # a forward without gradient issues the value-only launch behind the latent block's (and the statistics'); inference issues
        # nothing. 0 (the default): the launches as they were. store.class_mmd_acc is not undone by the step guards, as lat_stats.
        self.class_mmd, self.class_mmd_s2 = 0.0, None
        self.class_mmd_issued = None  # the form the sequence issued last took: None, 'value' or 'grad'
        self.class_mmd_rows = store.class_mmd_rows(B)  # (allocated here, never inside a capture)
        self.logits =None if self.forms.fuse_bce else act(B * T, cfg.out_dim)  # (fused: the logits never reach HBM)
        self.dlogits = act(B * T, cfg.out_dim)
        if cfg.kind == "token":
            self.probs = torch.zeros(B * T, cfg.out_dim, **f32) if want_probs else None
        else:
            self.probs = act(B * T, cfg.out_dim) if want_probs else None
        self.npos = torch.zeros(B, dtype=torch.int32, device=dev)

        # ---- backward temporaries (encoder and decoder sized separately)
        def bwd_bufs(M, D, H, S):
            t = _Layer()
            t.dx_a, t.dx_b = act(M, D), act(M, D)      # gradient w.r.t. a layer's output / input (ping-pong)
            t.dh, t.dhm = act(M, D), act(M, D)          # LN backward output and its dropout-masked copy
            t.dh1, t.dh1m = act(M, D), act(M, D)
            t.dpre, t.dx1 = act(M, 4 * D), act(M, D)
            t.datt, t.dqkv = act(M, D), act(M, 3 * D)
            t.delta = torch.zeros(B, H, S, **f32)
            return t

        # one set per layer: every weight gradient of the step is computed by ONE launch at the end of backward(), so the
        # operands it reads (dh, dpre, dh1, dqkv of each layer) must survive until then. (Running them on a forked
        # stream instead bought nothing: hipGraph on ROCm 7.2 replays fork/join branches back to back on one queue.)
        self.be_l = [bwd_bufs(self.Me, De, cfg.e_heads, Se) for _ in range(cfg.e_layers)]
        self.bd_l = [bwd_bufs(self.Md, Dd, cfg.d_heads, Sd) for _ in range(cfg.d_layers)]
        self._wgrads = []
        self.wgrad_scratch = store.wgrad_scratch()
        # LayerNorm parameter gradients: every LayerNorm-backward workgroup leaves one row of column sums here and ONE
        # launch per flush adds them into the bucket (256 workgroups x one atomic per column on the same 2D addresses
        # serialised for ~5 us per launch: 30 us of the step at configs[1])
        self._ln_part, self._psums = {}, []
        for side, n_l, M, D in (("encoder", cfg.e_layers, self.Me, De), ("decoder", cfg.d_layers, self.Md, Dd)):
            rows = max(o.layernorm_bwd_parts(M, D), o.gemm_nt_ln_parts(M))
            for i in range(n_l):
                for ln in ("ln1", "ln2" if side == "encoder" else "ln3"):
                    self._ln_part[f"{side}.layer{i}.{ln}"] = torch.zeros(rows, 2 * D, **f32)
        self.lat_scratch = torch.zeros(B * (Dd + 2 * Z), **f32)
        # Sparse gradient carriers, never used as ping-pong targets so their untouched rows stay zero:
        #   d_dec_out: d(decoder output) - rows 1..T written by the output-layer dgrad, row 0 always 0 (model.py:253)
        #   d_enc_out: d(encoder output) - only row 0 of each sample written, by latent_bwd_vec (model.py:97)
        self.d_dec_out = act(self.Md, Dd)
        self.d_enc_out = act(self.Me, De)
        # Top encoder layer, backward: the loss reads the encoder only at position 0 (model.py:97), so the gradient
        # entering the last layer is non-zero in B of its B*T rows, and LayerNorm / FFN / W_proj are row-wise: their
        # backward runs on those B rows (strided views), exactly. Only attention mixes rows; it gets its dO through
        # sp_datt and the residual branch through sp_dh1, full-size buffers whose other rows are never written.
        c = _Layer()
        c.dh, c.dhm, c.dx1, c.dh1m = act(B, De), act(B, De), act(B, De), act(B, De)
        c.dpre = act(B, 4 * De)
        self.sp_dh1 = c.dh1 = act(self.Me, De)
        self.sp_datt = c.datt = act(self.Me, De)
        c.dqkv, c.delta = self.be_l[-1].dqkv, self.be_l[-1].delta  # (attention mixes rows: the layer's own full-size buffers)
        self.top = c
        self.graph = None
        self.graph_late = None
        self.graph_opt = None
        self._tail_used = dict(fwd=False, bwd=False)  # which one-launch tails the kernel sequence issued last contains
        if o.can_row_tail(B, De) and store.tail_fused and not store.tail_checked:
            row_tail_selfcheck(store)

    # dropout probabilities of the current pass: 0 in inference mode (forward(inference=True)), where Dropout is the identity
    @property
    def e_p(self):
        return 0.0 if self._infer else self.cfg.e_dropout

    @property
    def d_p(self):
        return 0.0 if self._infer else self.cfg.d_dropout

    def _resolve_forms(self, with_grad=False):
        """Which form every launch of the sequence about to be issued takes: from the shape, and from the six attributes diagnostics
        set before the first forward() / capture() (store.tail_fused — which a failed tail also clears —, store.shadows_deferred,
        plan.ride, plan.shadows_on_tail, plan.dec_tail, plan.kqv_head). forward() resolves them; every phase of the step reads this record
        and nothing else. with_grad: the forward pass of a training step whose caller issues losses(with_grad=True) next (fwd_bwd_kernels)."""
        cfg, st, B, T = self.cfg, self.store, self.B, self.T
        De, Dd = cfg.e_model, cfg.d_model
        roll = cfg.kind == "pianoroll"
        # position-0 tails of the top encoder layer as one launch each (mst_row_tail_*), else five
        tails = bool(o.can_row_tail(B, De) and st.tail_fused)
        riders = bool(self.ride and tails)
        # the refresh of the transposed shadows (read by the backward pass only): 'own' launch behind the optimizer; deferred to the
        # next step, behind the forward 'tail''s riders where that launch has them — compute units that idle until the position-0
        # chain ends — else behind the tiles of the step's first launch ('begin', +4.9 us)
        shadows = "own" if not st.shadows_deferred else ("tail" if self.shadows_on_tail and riders else "begin")
        # output layer + BCE in one launch when a tile can hold whole rows of pitches of one sample (configs[1]: P 128, T 256)
        fuse_bce = roll and o.can_fuse_bce(cfg.out_dim, T, self.nld) and o.bce_fusion_pays(cfg.out_dim)
        ffn_d, ln_bwd_d = o.ffn_fusion_pays(Dd, 4 * Dd), o.ln_bwd_fusion_pays(Dd)
        bce_dgrad = fuse_bce and ln_bwd_d
        skip_row0 = cfg.d_layers > 0 and T % 64 == 0 and ffn_d
        return Forms(
            tails=tails, riders=riders, shadows=shadows, fuse_bce=fuse_bce,
            # ... and the output layer's input gradient + the last decoder layer's LayerNorm-3 backward in the same workgroups
            bce_dgrad=bce_dgrad,
            # The LAST decoder layer's row-wise part (W_proj, LayerNorm-1, feed-forward, LayerNorm-3 and their backward) skips every
            # sample's position-0 row: its output is dropped before the loss (model.py:253), so nothing it computes there is ever
            # read and every gradient there is zero — the buffers' position-0 rows simply stay at the zeros they were allocated with.
            # B x T rows are B T / 64 tiles of the one-workgroup-per-CU feed-forward launches: ONE resident round at configs[1]
            # (256 tiles) where B (T + 1) rows were 257 (measured: forward 22.8 -> 18.9 us, backward 24.6 -> 20.3).
            skip_row0=skip_row0,
            # ... and that block, the loss launch and the block's backward — three consecutive launches on the same 64-row tiles — as
            # consecutive phases of ONE launch's workgroups (mst_dec_tail_step). Only in a training step with gradient: forward()
            # then leaves the block to losses(with_grad=True); every other path keeps the three launches.
            dec_tail=bool(with_grad and not self._infer and self.dec_tail and bce_dgrad and ffn_d and skip_row0 and
                          o.dec_tail_pays(Dd, 4 * Dd, cfg.out_dim, T, B * T // 64, self.n_cu)),
            # The class-embedding gradient is a column sum of d(x0) per class = onehot(class)^T d(x0): with the one-hot class id
            # of a frame in C extra columns behind its pitches, and the class table behind the embedding table in the flat
            # buffers, it is rows in_dim.. of the encoder embedding's weight-gradient problem — whose 256-row tile has the
            # room — instead of a launch of its own (otherwise: the group_colsum launch)
            cls_fold=(roll and cfg.in_dim % 8 == 0 and roundup(cfg.in_dim + cfg.num_classes, 256) == roundup(cfg.in_dim, 256) and
                      st.offsets["encoder.class2hid.weight"] == st.offsets["encoder.embedding.weight"] + cfg.in_dim * De),
            # the row-wise block of a layer as one launch forward / backward (row_block_fwd / _bwd 'fused'), and Dense dgrad +
            # LayerNorm backward in one launch (row_block_bwd 'ln_fused', the chain of leading LayerNorm backwards: _out_ln_bwd)
            ffn_e=o.ffn_fusion_pays(De, 4 * De), ffn_d=ffn_d, ln_bwd_e=o.ln_bwd_fusion_pays(De), ln_bwd_d=ln_bwd_d,
            # training schedules: KL weight, free bits and lr warm-up from the device schedule block (training steps only — a
            # validation step keeps the constants: its objective must not move with the schedule)
            sched=self.scheduled,
            # clipping by the global gradient norm: a sum-of-squares launch ahead of Adam, the Adam launches in their gnorm form
            gnorm=self.clip_global_norm > 0,
            # the exponential moving average of the weights: the Adam launches in their averaging form
            ema=self.ema_decay > 0,
            # the W_proj input gradient inside the attention-backward launch, where the library takes the shape that way
            # (mst_attn_bwd_form; the causal decoder has kernels of its own)
            attn_proj_e=self._attn_proj(T, cfg.e_heads, De), attn_proj_d=not cfg.d_causal and self._attn_proj(T + 1, cfg.d_heads, Dd),
            # the K | Q | V input gradient of an encoder layer as the head of the one-launch backward block below it (which then starts
            # with its leading LayerNorm backward: row_block_bwd 'fused' with a lead), where the library takes the shape that way
            kqv_head_e=bool(self.kqv_head and cfg.e_layers >= 2 and o.ffn_fusion_pays(De, 4 * De) and not o.ln_bwd_fusion_pays(De) and
                            o.kqv_head_pays(self.adt, B * T, De)),
            # decoder-input dropout: the bookkeeping draws the keep mask (and writes the masked frames), the decoder's embedding and
            # its gradient read them. Training steps only: an inference pass and a validation step (is_train False) see every input —
            # their objective must not move with the option, and they are the launches of a plan without it
            in_drop=self.d_input_dropout > 0 and self._tick_adam and not self._infer)

    def _class_mmd_on(self):
        check_class_mmd(self.class_mmd, self.class_mmd_s2)
        return self.class_mmd > 0

    def _class_mmd_s2(self):
        """the kernel's bandwidth: E|z_i - z_j|^2 = 2 Z under the prior, so s2 = Z unless the caller chose one"""
        return float(self.class_mmd_s2) if self.class_mmd_s2 else float(self.cfg.latent_dim)

    def _attn_proj(self, S, H, D):
        return bool(o.attn_bwd_form(self.adt, self.B, S, H, D // H, 0, D, 2 * D, 3 * D, D, 3 * D, proj=True)["proj"])

    def _guard(self):
        """step guard of the launches that close a step (optimizer / loss_combine): the barrier counters of the one-launch
        tails issued in this step must have reached their final values"""
        fwd, bwd = o.row_tail_barriers(self.cfg.e_model)
        exp = []
        if self._tail_used["fwd"]:
            exp.append((self.sync_words[0:1], fwd))
        if self._tail_used["bwd"]:
            exp.append((self.sync_words[4:5], bwd))
        g = dict(status=self.store.step_status, expect=exp)
        if self.global_batch == self.B:
            # one rank: the optimizer also skips a step whose loss is not finite (its gradients are NaN: an update would destroy the
            # model). Not with more ranks: the loss is per rank, the all-reduced gradient is not — ranks would part ways.
            g["finite"] = (self.recon, self.kl)
        return g

    # ------------------------------------------------------------------------------ inputs
    def bind_inputs(self, buf):
        """Make `buf` (a device uint8 blob with pack_batch()'s layout) the step's input buffer: the typed views the
        kernels read are re-pointed, nothing is copied. A graph captured afterwards reads THAT buffer — a batcher that
        fills two or more such buffers in turn (or bench.py's resident batches) needs no device-to-device hop."""
        cfg, B, T = self.cfg, self.B, self.T
        need = max(a + n for a, n in self.in_layout.values())
        if not (buf.dtype == torch.uint8 and buf.is_contiguous() and buf.is_cuda and buf.data_ptr() % 16 == 0 and buf.numel() >= need):
            raise ValueError("bind_inputs: need a contiguous, 16-byte aligned device uint8 blob of pack_batch()'s size")
        self.inbuf = buf

        def inview(name, dtype, *shape):
            a, n = self.in_layout[name]
            return buf[a: a + n].view(dtype).view(*shape)

        if cfg.kind == "token":
            self.tokens = inview("tokens", torch.int32, B, T)
            self.labels = inview("labels", torch.int32, B, T)
        else:
            self.roll_cls = inview("roll", torch.uint8, B * T, self.ld_roll)  # [pitches | one-hot class | 0]
            self.roll = self.roll_cls[:, : roundup(cfg.in_dim, 8)]
            self.labels = inview("labels", torch.uint8, B * T, cfg.out_dim)
        self.seq_lens = inview("seq_lens", torch.int32, B)
        self.classes = inview("classes", torch.int32, B)

    def load_batch(self, x, seq_lens, classes, labels, eps=None):
        """Copy one batch (host or device tensors / numpy arrays) into the static input buffers."""
        def dev(a, dtype):
            t = torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a
            return t.to(device=self.dev, dtype=dtype, non_blocking=True)

        cfg, B, T = self.cfg, self.B, self.T
        if cfg.kind == "token":
            self.tokens.copy_(dev(x, torch.int32).view(B, T))
            self.labels.copy_(dev(labels, torch.int32).view(B, T))
        else:
            self.roll[:, : cfg.in_dim].copy_(dev(x, torch.uint8).view(B * T, cfg.in_dim))
            self.labels.copy_(dev(labels, torch.uint8).view(B * T, cfg.out_dim))
        self.seq_lens.copy_(dev(seq_lens, torch.int32))
        self.classes.copy_(dev(classes, torch.int32))
        if self.forms.cls_fold:
            w = self.ld_roll - cfg.in_dim
            onehot = (self.classes.view(B, 1).to(torch.int64) == torch.arange(w, device=self.dev).view(1, w)).to(torch.uint8)
            self.roll_cls.view(B, T, -1)[:, :, cfg.in_dim:].copy_(onehot.view(B, 1, w).expand(B, T, w))
        if eps is not None:
            self.eps.copy_(dev(eps, torch.float32))

    def pack_into(self, blob, x, seq_lens, classes, labels):
        """write one batch into `blob`, a HOST uint8 tensor with the layout of `inbuf` (a persistent page-locked staging
        buffer of PinnedBatchPipeline, or a fresh one from pack_batch); bytes between the segments are left alone.
        Plain numpy copies on the calling thread: a torch copy_ of a 2 MB tensor fans out over the intra-op thread pool,
        whose idle spinning (128 threads on a 16-core share of the GPU box) ran the process into its CPU quota — a stall
        of ~90 ms every few dozen batches."""
        cfg, B, T = self.cfg, self.B, self.T
        assert blob.dtype == torch.uint8 and not blob.is_cuda and blob.numel() >= self.inbuf.numel()
        raw = blob.numpy()

        def seg(name, dtype, *shape):
            a, n = self.in_layout[name]
            return raw[a: a + n].view(dtype).reshape(*shape)

        def as_np(a):
            return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)

        if cfg.kind == "token":
            np.copyto(seg("tokens", np.int32, B, T), as_np(x).reshape(B, T), casting="unsafe")
            np.copyto(seg("labels", np.int32, B, T), as_np(labels).reshape(B, T), casting="unsafe")
        else:
            ldp = self.ld_roll
            roll = seg("roll", np.uint8, B * T, ldp)
            np.copyto(roll[:, : cfg.in_dim], as_np(x).reshape(B * T, cfg.in_dim), casting="unsafe")
            if self.forms.cls_fold:
                w = ldp - cfg.in_dim
                roll.reshape(B, T, ldp)[:, :, cfg.in_dim:] = (as_np(classes).reshape(B, 1, 1).astype(np.int64) ==
                                                              np.arange(w).reshape(1, 1, w)).astype(np.uint8)
            elif ldp != cfg.in_dim:
                roll[:, cfg.in_dim:] = 0
            np.copyto(seg("labels", np.uint8, B * T, cfg.out_dim), as_np(labels).reshape(B * T, cfg.out_dim), casting="unsafe")
        np.copyto(seg("seq_lens", np.int32, B), as_np(seq_lens).reshape(B), casting="unsafe")
        np.copyto(seg("classes", np.int32, B), as_np(classes).reshape(B), casting="unsafe")
        return blob

    def pack_batch(self, x, seq_lens, classes, labels):
        """a fresh host blob with the layout of `inbuf` (what bench.py keeps resident after one upload)"""
        return self.pack_into(torch.zeros(self.inbuf.numel(), dtype=torch.uint8), x, seq_lens, classes, labels)

    def load_packed(self, blob):
        """one copy (host->device or device->device) of a pack_batch() blob into the step's input buffers"""
        self.inbuf.copy_(blob, non_blocking=True)

    # ------------------------------------------------------------------------------ forward
    def _drop(self, p, site):
        return dict(dropout_p=p, dropout_site=site, dropout_seed_ptr=self.rng_state) if p > 0 else {}

    def _dropout(self, p, site0):
        return Dropout(p, self.rng_state if p > 0 else None, site0)

    def _site_e(self, i):
        """first of the three dropout site ids of encoder layer i (attention output, FFN hidden, FFN output)"""
        return self.site_base + 3 * i

    def _site_d(self, i):
        return self.site_base + 3 * (self.cfg.e_layers + i)

    def _late_shadows(self):
        """the deferred refresh of the transposed shadows only the backward pass reads (ParamStore.shadows_deferred)"""
        st = self.store
        return dict(w=st.w, wt16=st.wt16, desc=st.t_desc_late, prefix=st.t_prefix_late, n_mat=st.t_n_late, tiles=st.t_tiles_late)

    def _top_encoder_layer_fwd(self, i, L, x_in):
        """Last encoder layer: the model reads its output at position 0 only (model.py:97) and everything after the
        attention mix is row-wise, so after the dense K/Q/V projection and the softmax row statistics (which
        normalise over ALL queries) only query 0 is attended and only B rows go through W_proj, LN1, the FFN and LN2.
        The other rows of these buffers are never produced nor read (backward: _top_encoder_layer_bwd)."""
        cfg, st, B, S, F = self.cfg, self.store, self.B, self.T, self.forms
        D, H = cfg.e_model, cfg.e_heads
        P = st.layer("encoder", i)
        # (the K | Q | V projection runs inside the attention launch where the shape allows: mst_attn_qkv_fwd)
        o.attn_qkv_fwd(x_in, P.kqv.w, P.kqv.b, L.qkv, self.keymask_e, L.lse, L.att, B, S, H, D // H, 0, D, 2 * D, q_limit=1)
        self._tail_used["fwd"] = F.tails
        tail = None
        if F.tails:
            tail = dict(sync=self.sync_words[0:3], stat_stride=S, phys_stride=S, status=st.step_status[0:1], queue=self.ride_queues[0:1])
            if F.riders:  # the decoder's first K | Q | V projection, rows 1..T of every sample (see __init__: ride)
                Pd, Dd, Sd = st.layer("decoder", 0), cfg.d_model, S + 1
                tail["rider"] = dict(A=self.x0_d, B=Pd.kqv.w, C_out=self.dec[0].qkv, M=B * S, N=3 * Dd, K=Dd, bias=Pd.kqv.b,
                                     a_remap=(S, Sd, 1), c_remap=(S, Sd, 1))
                if F.shadows == "tail":
                    tail["shadows"] = self._late_shadows()
        return row_block_fwd(P, L, x_in, position0_rows(B, S), self._dropout(self.e_p, self._site_e(i)),
                             "tail" if F.tails else "launches", tail=tail)

    def _layer_fwd(self, side, i, L, x_in, keymask, D, H, S, p, site0):
        F = self.forms
        dh = D // H
        if side == "encoder" and i == self.cfg.e_layers - 1:
            return self._top_encoder_layer_fwd(i, L, x_in)
        P = self.store.layer(side, i)
        causal = side == "decoder" and self.cfg.d_causal
        if side == "decoder" and i == 0 and F.riders:  # (projected by the forward tail's riders + the latent block's launch)
            (o.attn_causal_fwd if causal else o.attn_fwd)(L.qkv, keymask, L.lse, L.att, self.B, S, H, dh, 0, D, 2 * D)
        elif causal:  # the projection GEMM, then the causal attention launch
            o.gemm_nt(x_in, P.kqv.w, L.qkv, N=3 * D, K=D, bias=P.kqv.b)
            o.attn_causal_fwd(L.qkv, keymask, L.lse, L.att, self.B, S, H, dh, 0, D, 2 * D)
        else:
            o.attn_qkv_fwd(x_in, P.kqv.w, P.kqv.b, L.qkv, keymask, L.lse, L.att, self.B, S, H, dh, 0, D, 2 * D)
        fused = F.ffn_e if side == "encoder" else F.ffn_d
        if F.dec_tail and side == "decoder" and i == self.cfg.d_layers - 1:
            return L.x2  # (the block runs inside the loss launch: losses())
        return row_block_fwd(P, L, x_in, ALL_ROWS, self._dropout(p, site0), "fused" if fused else "launches",
                             row_groups=self._row0_groups(side, i))

    def _row0_groups(self, side, i):
        """row groups of the last decoder layer's row-wise launches (Forms.skip_row0, which implies their fused form): rows 1..T of
        every T + 1, else None"""
        if side == "decoder" and i == self.cfg.d_layers - 1 and self.forms.skip_row0:
            return (self.T, self.T + 1, 1)
        return None

    def forward(self, inference=False, upto=None, with_grad=False, start=None):
        """inference=True: the forward pass as the reference runs it OUTSIDE autograd.record() (Model(...) called directly, the
        samplers: sampler.py:146-148) — every Dropout is the identity and the training RNG stream is left alone (an eps the
        caller did not supply is drawn from the store's inference stream).
        upto="latent" (inference only): stop behind the latent launch — mu, sigma, z and decoder row 0 are there, no decoder layer,
        output layer or loss launch is issued (Model.encode).
        with_grad=True (fwd_bwd_kernels, a training step): the caller issues losses(with_grad=True) next — where Forms.dec_tail holds,
        the last decoder layer's row-wise block is left to that launch and dec_out is filled by it, not by forward().
        start="latent" (inference only): a DRAW PASS — the decoder half alone, on the encoder output the preceding full inference forward
        of this plan left (IWBound). One bookkeeping launch of its own (a new seed and eps from the store's inference stream for a plan
        with internal_eps, the recon buffer cleared), the latent launch, the decoder layers and the output layer: no encoder launch.
        Rows 1..T of the decoder input do not depend on z and no decoder launch writes them, so they are reused, as is — where the
        forward tail's riders made it — the first K | Q | V projection of those rows. start=None issues the launches it always did."""
        if with_grad and (inference or upto or start):
            raise ValueError("forward(with_grad=True) is the forward pass of a training step")
        if start not in (None, "latent") or (start and (not inference or upto)):
            raise ValueError("forward(start=...) takes 'latent', in inference mode and without upto")
        if start and getattr(self, "enc_out", None) is None:
            raise RuntimeError("forward(start='latent') needs the encoder output of a preceding full forward(inference=True) of this plan")
        if upto not in (None, "latent") or (upto and not inference):
            raise ValueError("forward(upto=...) takes 'latent', in inference mode only")
        cfg, st, B, T = self.cfg, self.store, self.B, self.T
        self._infer = bool(inference)
        # (every forward: handle_step_status() may have cleared store.tail_fused since the last one. losses(), the backward phases and
        # optimizer() — also when captured as graphs of their own — read the record this forward leaves.)
        F = self.forms = self._resolve_forms(with_grad)
        self._tail_used = dict(fwd=False, bwd=False)
        self.class_mmd_issued = None
        De, Dd = cfg.e_model, cfg.d_model
        Se, Sd = T, T + 1
        sq_e, sq_d = math.sqrt(float(De)), math.sqrt(float(Dd))
        self._wgrads, self._psums, self._outers, self._cls_job = [], [], [], None  # deferred gradient work of this step
        # one bookkeeping launch: RNG seed of this step, Adam's step count / lr_t, eps, both padding masks
        need_rng = self.e_p > 0 or self.d_p > 0 or self.internal_eps or F.in_drop
        rng = st.rng_state_inference() if self._infer else self.rng_state
        tick = self._tick_adam and not self._infer
        begin = dict(rng_state=rng if need_rng else None,
                     adam_state=st.step_state if tick else None, lr=self.lr, beta1=self.opt["beta1"],
                     beta2=self.opt["beta2"], eps_out=self.eps if self.internal_eps else None,
                     eps_index0=self.sample_offset * cfg.latent_dim, lens=self.seq_lens,
                     mask_e=self.keymask_e if cfg.kind != "token" else None, add_e=0, mask_d=self.keymask_d, add_d=1,
                     zero_a=self._recon_buf, zero_b=st.g if tick else None)
        if F.shadows == "begin":
            begin["shadows"] = self._late_shadows()
        if F.sched and tick:  # the thread that ticks Adam writes this step's schedule block
            begin["schedule"] = dict(block=st.sched, kl_weight=self.kl_weight, **self.schedule)
        roll_d = keep_d = None  # what the decoder's embedding reads in place of `roll` / besides the tokens
        if F.in_drop:
            # position k of sample b (the input of decoder row k + 1) is draw number (sample_offset + b) * T + k of the step's stream:
            # per GLOBAL sample index, like eps (mst_step_begin_args.in_*)
            begin["input_drop"] = dict(keep=self.in_keep, p=self.d_input_dropout, index0=self.sample_offset * T)
            keep_d = self.in_keep
            if cfg.kind != "token":
                roll_d = self.roll_d
                begin["input_drop"].update(src=self.roll, dst=roll_d)  # (the bound blob's frames: bind_inputs)
        # (piano-roll ends: nothing in the embedding GEMMs reads what the bookkeeping writes — it rides on their launch)
        ride = cfg.kind != "token" and not start
        if start:  # the draw pass's own bookkeeping: seed + eps, the recon buffer; masks and decoder rows 1..T stand as they are
            o.step_begin(rng_state=begin["rng_state"], eps_out=begin["eps_out"], eps_index0=begin["eps_index0"], zero_a=self._recon_buf)
        elif not ride:
            o.step_begin(**begin)
        # ---- encoder input (model.py:81-91, transformer.py:270)
        if start:
            pass
        elif cfg.kind == "token":
            o.embed_fwd(self.tokens, st.p("encoder.embedding.weight"), self.pos_e, self.x0_e.view(B, Se, -1), 0, sq_e,
                        classes=self.classes, cls_table=st.p("encoder.class2hid.weight"), keymask=self.keymask_e)
        else:
            # both ends' embedding GEMMs read the same frames: one launch (the decoder's rows 1..T; its row 0 is latent_fwd's)
            o.gemm_nt_pair(dict(A=self.roll, B=st.t("encoder.embedding.weight"), C_out=self.x0_e, N=De, alpha=sq_e,
                                grpadd=st.p("encoder.class2hid.weight"), grp_index=self.classes, rowadd=self.pos_e, rowadd_period=T),
                           dict(A=roll_d if F.in_drop else self.roll, B=st.t("decoder.embedding.weight"), C_out=self.x0_d, M=B * T, N=Dd,
                                alpha=sq_d,
                                rowadd=self.pos_d[1:], rowadd_period=T, c_remap=(T, Sd, 1)),
                           begin=begin if ride else None)
        x = self.enc_out if start else self.x0_e
        for i, L in enumerate(() if start else self.enc):
            x = self._layer_fwd("encoder", i, L, x, self.keymask_e, De, cfg.e_heads, Se, self.e_p, self._site_e(i))
        self.enc_out = x
        # ---- latent block + decoder position 0 (model.py:97-103,292,229-232)
        lat = (x.view(B, Se, -1), st.p("encoder.latent_proj.weight"), st.p("encoder.latent_proj.bias"), self.eps,
               st.p("decoder.latent2hid.weight"), st.p("decoder.latent2hid.bias"), self.classes,
               st.p("decoder.class2hid.weight"), self.pos_d, sq_d, self.mu, self.sigma, self.z, self.kl,
               self.x0_d.view(B, Sd, -1))
        # (the decoder's first K | Q | V projection riding on this launch — rows 1..T exist since the step's first launch — was
        # built and measured at parity: 16-wave workgroups make poor GEMM tiles at K = 128; removed, docs/kernel_notes.md)
        proj0 = None
        if F.riders:  # ... and position 0 of that projection, on the launch that produces the row
            Pd = st.layer("decoder", 0)
            proj0 = (Pd.kqv.w, Pd.kqv.b, self.dec[0].qkv.view(B, Sd, -1))
        o.latent_fwd(*lat, proj=proj0)
        if self.track_latent_stats and not self._infer:
            o.latent_dim_stats(self.mu, self.sigma, self.classes, st.lat_stats)
        if self._class_mmd_on() and not self._infer and not with_grad:  # (a training step: behind the latent backward, backward_early)
            o.class_mmd(self.z, self.classes, self._class_mmd_s2(), self.class_mmd_rows, st.class_mmd_ticket, st.class_mmd_acc)
            self.class_mmd_issued = "value"
        if upto == "latent":
            return
        # ---- decoder positions 1..T (model.py:241-245, transformer.py:237)
        if cfg.kind == "token" and not start:
            o.embed_fwd(self.tokens, st.p("decoder.embedding.weight"), self.pos_d, self.x0_d.view(B, Sd, -1), 1, sq_d, keep=keep_d)
        x = self.x0_d
        site_d = self._site_d(0)
        for i, L in enumerate(self.dec):
            x = self._layer_fwd("decoder", i, L, x, self.keymask_d, Dd, cfg.d_heads, Sd, self.d_p, site_d + 3 * i)
        self.dec_out = x
        # ---- output layer on positions 1..T (model.py:253-256); with a whole row of pitches per tile it runs inside the loss
        # launch (losses(): mst_gemm_sigmoid_bce) and the logits never reach HBM
        if not F.fuse_bce:
            o.gemm_nt(x, st.h("decoder.output_layer.weight"), self.logits, M=B * T, K=Dd, bias=st.p("decoder.output_layer.bias"),
                      a_remap=(T, Sd, 1))

    def losses(self, with_grad=True, combine=True, plain=False):
        """combine=False: the total loss / running metric sums are left to optimizer() (they ride on the Adam launch).
        plain=True (without gradient: IWBound): the plain likelihood whatever the training configuration says — label smoothing 0,
        down-weighting off — and nothing added to the trainer's token / piano-roll metric sums"""
        cfg, B, T, F = self.cfg, self.B, self.T, self.forms
        if plain and with_grad:
            raise ValueError("losses(plain=True) is a likelihood, not a training loss: with_grad=False")
        ls, nld = (0.0, False) if plain else (self.ls, self.nld)
        dl = self.dlogits if with_grad else None
        counts = self.store.roll_counts if self.track_roll_metrics and not plain else None
        if cfg.kind == "token":
            o.softmax_ce(self.logits, self.labels, self.recon, B, T, cfg.out_dim, probs=self.probs, dlogits=dl,
                         gscale=self.gscale, pre_zeroed=True,
                         tok_parts=self.store.tok_parts if self.track_token_metrics and not plain else None)
        elif F.fuse_bce:
            dgrad = None
            if F.dec_tail and not with_grad:
                raise RuntimeError("forward(with_grad=True) left the last decoder layer to losses(with_grad=True)")
            if with_grad and F.bce_dgrad:
                # the first launch of the backward pass — the output layer's input gradient + the last decoder layer's LayerNorm-3
                # backward (backward_early) — consumes exactly the logit-gradient tile this launch produces: same workgroup
                last, Dd, Sd = cfg.d_layers - 1, cfg.d_model, T + 1
                dgrad = dict(A=self.dlogits, B=self.store.t("decoder.output_layer.weight"), dX_out=self.bd_l[last].dh, M=B * T, N=Dd,
                             K=self.dlogits.shape[1], c_remap=(T, Sd, 1),
                             **self._out_ln_bwd("decoder", last, self.dec[last], cfg.d_dropout, self._site_d(0) + 3 * last,
                                                self.bd_l[last], B * T))
            loss = dict(A=self.dec_out, B=self.store.h("decoder.output_layer.weight"), labels=self.labels, loss=self.recon, T=T,
                        dlogits=dl, probs=self.probs, label_smoothing=ls, downweight=nld, gscale=self.gscale, M=B * T,
                        K=cfg.d_model, bias=self.store.p("decoder.output_layer.bias"), a_remap=(T, T + 1, 1), counts=counts)
            if F.dec_tail:
                # ... and around it, in the same workgroups again, the last decoder layer's row-wise block (forward() left it out) and
                # that block's backward (backward_early skips its launch, and registers its partial sums and weight gradients as ever)
                L, t, P = self.dec[last], self.bd_l[last], self.store.layer("decoder", last)
                drop, groups = self._dropout(self.d_p, self._site_d(0) + 3 * last), self._row0_groups("decoder", last)
                x_in = self.dec[last - 1].x2 if last > 0 else self.x0_d
                o.dec_tail_step(row_block_fwd(P, L, x_in, ALL_ROWS, drop, "fused", row_groups=groups, launch=False), loss, dgrad,
                                ffn_bwd_kw(P, L, t, drop, self._ln_partials_buf(P.ln1, ffn_bwd_parts(L, groups)), groups))
            else:
                o.gemm_sigmoid_bce(dgrad=dgrad, **loss)
        else:
            o.sigmoid_bce(self.logits, self.labels, self.recon, B, T, cfg.out_dim, label_smoothing=ls,
                          downweight=nld, npos=self.npos, probs=self.probs, dlogits=dl, gscale=self.gscale,
                          pre_zeroed=True, counts=counts)
        if combine:
            o.loss_combine(self.recon, self.kl, self.kl_weight, self.total, self.metric_acc, guard=self._guard())

    # ------------------------------------------------------------------------------ backward
    LN_PARTIALS_MIN = 32  # fewer workgroups than this: their atomics are cheaper than a row of partials each

    def _ln_partials_buf(self, norm, parts):
        """the buffer _ln_partials hands out, without registering anything"""
        return self._ln_part[norm.site] if parts >= self.LN_PARTIALS_MIN else None

    def _ln_partials(self, norm, parts):
        """partials buffer of one LayerNorm-backward launch of `parts` workgroups (None: few workgroups, keep the atomics); registers
        the deferred column sums into dgamma / dbeta, executed by _flush_grads()"""
        buf, dg, db = self._ln_partials_buf(norm, parts), norm.dgamma, norm.dbeta
        if buf is None:
            return None
        D = dg.numel()
        if db.data_ptr() == dg.data_ptr() + 4 * D:  # adjacent in the flat bucket: one job
            self._psums.append(o.partial_sum_job(buf, parts, dg, length=2 * D))
        else:
            self._psums += [o.partial_sum_job(buf, parts, dg, length=D), o.partial_sum_job(buf, parts, db, col_off=D, length=D)]
        return buf

    def _flush_grads(self):
        """the weight gradients collected so far in one wgrad launch; the LayerNorm column sums ride on its reduction pass"""
        o.gemm_wgrad_batch(self._wgrads, scratch=self.wgrad_scratch, sums=self._psums, outers=self._outers, cls=self._cls_job)
        self.last_wgrad_launch = (self._wgrads, self._psums)  # (bench.py re-launches the step's own wgrad batch to time it)
        self._wgrads, self._psums, self._outers, self._cls_job = [], [], [], None

    def _out_ln_bwd(self, side, i, L, p, site0, t, M):
        """The LayerNorm backward a layer's backward pass STARTS with (LN2 of an encoder layer, LN3 of a decoder layer),
        as keyword arguments for ops.gemm_nt_ln_bwd: the GEMM (of M rows) that produces the layer's incoming gradient runs
        it in its epilogue (dX_out = t.dh) when the row width allows, see _layer_bwd(dy_done=...)."""
        P = self.store.layer(side, i)
        return dict(x=L.h2, gamma=P.ln2.gamma, mean=L.mean2, rstd=L.rstd2, dgamma=P.ln2.dgamma, dbeta=P.ln2.dbeta,
                    partials=self._ln_partials(P.ln2, o.gemm_nt_ln_parts(M)), **_lead_mask(P, t, self._dropout(p, site0)))

    def _kqv_dgrad(self, P, t, dx_in, next_ln, hand_down):
        """Who forms a layer's K | Q | V input gradient t.dqkv W_kqv + t.dh1 (t: the layer's backward buffers, or the top encoder
        layer's position-0 set): with next_ln, the GEMM that runs the leading LayerNorm backward of the layer below in its epilogue
        instead of writing dx_in; with hand_down (Forms.kqv_head_e), the one-launch block of the layer below, in front of its leading
        LayerNorm backward — nothing is issued, the GEMM is returned for it; else the plain GEMM into dx_in. Returns None unless handed down."""
        D = P.proj.w.shape[0]
        if next_ln is not None:
            kw, t_below = next_ln
            o.gemm_nt_ln_bwd(t.dqkv, P.kqv.t, t_below.dh, N=D, K=3 * D, resid=t.dh1, **kw)
        elif hand_down:
            return dict(A=t.dqkv, B=P.kqv.t, resid=t.dh1, N=D, K=3 * D)
        else:
            o.gemm_nt(t.dqkv, P.kqv.t, dx_in, N=D, K=3 * D, resid=t.dh1)
        return None

    def _layer_bwd(self, side, i, L, x_in, dy, dx_in, keymask, D, H, S, p, site0, t, dy_done=False, next_ln=None, ride=False, head=None):
        """dy: gradient w.r.t. the layer output x2; writes the gradient w.r.t. x_in into dx_in.
        dy_done: the producer of dy already ran this layer's leading LayerNorm backward (t.dh / t.dhm are filled).
        next_ln: (_out_ln_bwd(...) of the layer below, its scratch): run THAT layer's leading LayerNorm backward in the
        epilogue of this layer's last GEMM instead of writing dx_in.
        ride (decoder layer 0 when the backward tail takes a rider): rows 1..T of dx_in — which only the decoder embedding's weight
        gradient reads — are left to that launch and row 0 to the latent block's backward launch; returns (the rider's GEMM,
        latent_bwd_vec's proj= triple) for backward_early to hand them on.
        head (Forms.kqv_head_e): the K | Q | V dgrad the layer ABOVE left to this layer's one-launch block (row_block_bwd head=; dy is not
        read). An encoder layer above another one leaves its own the same way and returns it: dx_in is not written. Else returns None."""
        F, P = self.forms, self.store.layer(side, i)
        ffn, ln = (F.ffn_e, F.ln_bwd_e) if side == "encoder" else (F.ffn_d, F.ln_bwd_d)
        # (Forms.dec_tail: the last decoder layer's one-launch block already ran inside the loss launch, losses())
        in_loss = F.dec_tail and side == "decoder" and i == self.cfg.d_layers - 1
        proj = F.attn_proj_e if side == "encoder" else F.attn_proj_d
        dff, dproj = row_block_bwd(P, L, t, dy, ALL_ROWS, self._dropout(p, site0), "fused" if ffn else ("ln_fused" if ln else "launches"),
                                   self._ln_partials, dy_done=dy_done, row_groups=self._row0_groups(side, i), launch=not in_loss,
                                   proj_dgrad=not proj, head=head)
        if side == "decoder" and self.cfg.d_causal:
            o.attn_causal_bwd(L.qkv, keymask, L.lse, t.datt, t.dqkv, t.delta, self.B, S, H, D // H, 0, D, 2 * D)
        elif proj:  # dO = dproj W_proj is formed by the (batch, head) workgroups themselves; nothing else reads t.datt
            o.attn_proj_bwd(L.qkv, keymask, L.lse, dproj, P.proj.t, t.dqkv, t.delta, self.B, S, H, D // H, 0, D, 2 * D)
        else:
            o.attn_bwd(L.qkv, keymask, L.lse, t.datt, t.dqkv, t.delta, self.B, S, H, D // H, 0, D, 2 * D)
        if ride:  # (decoder layer 0: no layer below it to take the gradient in either other way)
            T_ = self.T
            handed = (dict(A=t.dqkv, B=P.kqv.t, C_out=dx_in, M=self.B * T_, N=D, K=3 * D, resid=t.dh1, resid_phys=True,
                           a_remap=(T_, T_ + 1, 1), c_remap=(T_, T_ + 1, 1)),
                      (t.dqkv.view(self.B, S, -1), P.kqv.t, t.dh1.view(self.B, S, -1)))
        else:
            handed = self._kqv_dgrad(P, t, dx_in, next_ln, side == "encoder" and i > 0 and F.kqv_head_e)
        # the layer's four weight gradients: deferred to the ONE wgrad launch at the end of backward() (their operands
        # live in this layer's own scratch `t` and in the forward activations, so nothing is overwritten meanwhile)
        self._wgrads += layer_wgrads(P, L, t, x_in, dff, dproj, ALL_ROWS)
        return handed

    def _top_encoder_layer_bwd(self, i, L, x_in, dx_in, next_ln=None, rider=None):
        """_layer_bwd for the LAST encoder layer, on the B rows (position 0 of each sample) that carry gradient: LayerNorm-2 backward,
        both FFN dgrads, LayerNorm-1 backward and the W_proj dgrad of those rows as one launch (with `rider`, a GEMM for its idle
        workgroups) or five; then attention backward (dO is zero outside position 0), the K | Q | V dgrad and the layer's deferred
        weight gradients. With Forms.kqv_head_e and a layer below, the K | Q | V dgrad is not issued here: it is left in self._kqv_head
        for backward_late's first _layer_bwd (dx_in is not written)."""
        cfg, st, B, S, F = self.cfg, self.store, self.B, self.T, self.forms
        D, H = cfg.e_model, cfg.e_heads
        P, c, rows = st.layer("encoder", i), self.top, position0_rows(B, S)
        self._tail_used["bwd"] = F.tails
        tail = None
        if F.tails:
            tail = dict(sync=self.sync_words[4:7], stat_stride=S, phys_stride=S, status=st.step_status[0:1], rider=rider,
                        queue=self.ride_queues[32:33])
        dff, dproj = row_block_bwd(P, L, c, self.d_enc_out, rows, self._dropout(cfg.e_dropout, self._site_e(i)),
                                   "tail" if F.tails else "launches", no_partials, tail=tail)
        # d(attention output): rows b*S of a buffer that is zero elsewhere
        o.attn_bwd(L.qkv, self.keymask_e, L.lse, c.datt, c.dqkv, c.delta, B, S, H, D // H, 0, D, 2 * D, q_limit=1)
        # (handed down: to the one-launch block of the layer below, the first launch of backward_late)
        self._kqv_head = self._kqv_dgrad(P, c, dx_in, next_ln, i > 0 and F.kqv_head_e)
        self._wgrads += layer_wgrads(P, L, c, x_in, dff, dproj, rows)

    def backward(self):
        self.backward_early(flush=False)
        self.backward_late()

    def grad_cut(self):
        """Offset that splits the flat gradient bucket by the time its entries are final: [cut, n) — the top encoder
        layer, latent_proj and every decoder tensor — is complete after backward_early(flush=True); [0, cut) — the
        remaining encoder layers, the encoder embedding and class table — after backward_late(). 0 when the encoder has
        a single layer (nothing is early)."""
        cfg, st = self.cfg, self.store
        if cfg.e_layers < 2:
            return 0
        return st.offsets[f"encoder.layer{cfg.e_layers - 1}.att.W_k.weight"]

    def _below(self, side, i, fuse):
        """_layer_bwd's next_ln for layer i of a stack: the leading LayerNorm backward of layer i - 1, where the fusion pays"""
        if not (fuse and i > 0):
            return None
        if side == "encoder":
            layers, bufs, p, site0, M = self.enc, self.be_l, self.cfg.e_dropout, self._site_e(i - 1), self.Me
        else:
            layers, bufs, p, site0, M = self.dec, self.bd_l, self.cfg.d_dropout, self._site_d(i - 1), self.Md
        return self._out_ln_bwd(side, i - 1, layers[i - 1], p, site0, bufs[i - 1], M), bufs[i - 1]

    def backward_early(self, flush):
        """Output layer, decoder, latent block and the TOP encoder layer. With `flush` the weight gradients collected so
        far get their own wgrad launch, so that the [grad_cut(), n) part of the bucket can be all-reduced while
        backward_late() runs (data parallel); without it they wait for the single launch at the end."""
        cfg, st, B, T, F = self.cfg, self.store, self.B, self.T, self.forms
        De, Dd = cfg.e_model, cfg.d_model
        Se, Sd = T, T + 1
        sq_d = math.sqrt(float(Dd))
        # (the gradient bucket was cleared by forward()'s bookkeeping, which also emptied the lists of deferred gradient work)
        # ---- output layer (rows 1..T of the decoder output; row 0 of dx_a stays zero)
        ldv = self.dlogits.shape[1]
        site_d = self._site_d(0)
        last = cfg.d_layers - 1
        if F.bce_dgrad:  # (it rode on the loss launch: losses())
            pass
        elif F.ln_bwd_d:  # output-layer dgrad + the last decoder layer's LayerNorm-3 backward (rows 1..T; row 0 of dh stays 0)
            o.gemm_nt_ln_bwd(self.dlogits, st.t("decoder.output_layer.weight"), self.bd_l[last].dh, M=B * T, N=Dd, K=ldv,
                             c_remap=(T, Sd, 1),
                             **self._out_ln_bwd("decoder", last, self.dec[last], cfg.d_dropout, site_d + 3 * last, self.bd_l[last], B * T))
        else:
            o.gemm_nt(self.dlogits, st.t("decoder.output_layer.weight"), self.d_dec_out, M=B * T, N=Dd, K=ldv, c_remap=(T, Sd, 1))
        self._wgrads.append(o.wgrad_problem(self.dlogits, self.dec_out, st.grad("decoder.output_layer.weight"),
                                            st.grad("decoder.output_layer.bias"), M=B * T, N=cfg.out_dim, K=Dd, b_remap=(T, Sd, 1)))
        dy, pingpong, handed = self.d_dec_out, (self.bd_l[0].dx_a, self.bd_l[0].dx_b), None
        for n, i in enumerate(reversed(range(cfg.d_layers))):
            x_in = self.dec[i - 1].x2 if i > 0 else self.x0_d
            handed = self._layer_bwd("decoder", i, self.dec[i], x_in, dy, pingpong[n % 2], self.keymask_d, Dd, cfg.d_heads, Sd,
                                     cfg.d_dropout, site_d + 3 * i, self.bd_l[i], dy_done=F.ln_bwd_d,
                                     next_ln=self._below("decoder", i, F.ln_bwd_d), ride=F.riders and i == 0)
            dy = pingpong[n % 2]
        d_x0_d = dy  # gradient w.r.t. the decoder input [B, Sd, Dd]
        rider, dx0 = handed or (None, None)
        # ---- decoder input: rows 1..T -> embedding, row 0 -> latent block
        if cfg.kind == "token":
            o.embed_bwd(self.tokens, st.grad("decoder.embedding.weight"), d_x0_d.view(B, Sd, -1), 1, sq_d,
                        keep=self.in_keep if F.in_drop else None)
        else:  # (Forms.in_drop: the frames the forward pass read, dropped rows zeroed)
            self._wgrads.append(o.wgrad_problem(self.roll_d if F.in_drop else self.roll, d_x0_d, st.grad("decoder.embedding.weight"),
                                                M=B * T, N=cfg.out_dim, K=Dd, scale=sq_d, b_remap=(T, Sd, 1)))
        # gradient w.r.t. the encoder output: zero except position 0 of every sample
        d_enc = self.d_enc_out
        # nothing but the optimizer reads the latent block's parameter gradients: they ride on the weight-gradient flush (extra
        # workgroups of its reduction pass) instead of being a launch in the middle of the backward pass's dependent chain — the
        # decoder class table's too (dcls_d None: no class-table launch behind the latent block's), as the flush's class-table job
        o.latent_bwd_vec(st.p("encoder.latent_proj.weight"), self.eps, st.p("decoder.latent2hid.weight"), self.classes, self.mu,
                         self.sigma, d_x0_d.view(B, Sd, -1), sq_d, self.kl_weight, self.gscale_enc,
                         None, d_enc.view(B, Se, -1), self.lat_scratch,
                         enc_scale=self.gscale_enc / self.gscale, proj=dx0, sched=(st.sched, self.kl) if F.sched else None)
        if self._class_mmd_on():
            # lambda * L joins the objective: its gradient is added to d[mu | sigma] (which the flush's outer products read later) and,
            # through Wl, to d(enc_out). The bucket holds sums over samples at the encoder-side scale, rescaled by
            # 1 / (global_batch * gscale) at the optimizer: coef = lambda * B * gscale_enc (each rank penalises its own shard)
            Z = cfg.latent_dim
            o.class_mmd(self.z, self.classes, self._class_mmd_s2(), self.class_mmd_rows, st.class_mmd_ticket, st.class_mmd_acc,
                        grad=dict(eps=self.eps, coef=float(self.class_mmd) * B * self.gscale_enc, Wl=st.p("encoder.latent_proj.weight"),
                                  dlat=self.lat_scratch[B * Dd: B * (Dd + 2 * Z)].view(B, 2 * Z), d_enc_out3=d_enc.view(B, Se, -1)))
            self.class_mmd_issued = "grad"
        self._cls_job = o.class_job(self.classes, self.lat_scratch, st.grad("decoder.class2hid.weight"), B, Dd)
        self._outers += o.latent_outer_jobs(self.lat_scratch, self.enc_out.view(B, Se, -1), self.z,
                                            st.grad("encoder.latent_proj.weight"), st.grad("encoder.latent_proj.bias"),
                                            st.grad("decoder.latent2hid.weight"), st.grad("decoder.latent2hid.bias"))
        top = cfg.e_layers - 1
        x_in = self.enc[top - 1].x2 if top > 0 else self.x0_e
        self._top_encoder_layer_bwd(top, self.enc[top], x_in, self.be_l[0].dx_a, next_ln=self._below("encoder", top, F.ln_bwd_e),
                                    rider=rider)
        if flush and cfg.e_layers >= 2:
            self._flush_grads()

    def backward_late(self):
        """The encoder layers below the top one, the encoder input, and the (remaining) weight gradients."""
        cfg, st, B, T, F = self.cfg, self.store, self.B, self.T, self.forms
        De, Se = cfg.e_model, T
        sq_e = math.sqrt(float(De))
        dy, pingpong = self.be_l[0].dx_a, (self.be_l[0].dx_b, self.be_l[0].dx_a)  # the top layer wrote dx_a
        # (F.ln_bwd_e: every layer's leading LayerNorm backward already ran in the GEMM above it)
        head = self._kqv_head  # (Forms.kqv_head_e: the top layer's K | Q | V dgrad, formed by the launch that reads it)
        for n, i in enumerate(reversed(range(cfg.e_layers - 1))):
            x_in = self.enc[i - 1].x2 if i > 0 else self.x0_e
            head = self._layer_bwd("encoder", i, self.enc[i], x_in, dy, pingpong[n % 2], self.keymask_e, De, cfg.e_heads, Se, cfg.e_dropout,
                                   self._site_e(i), self.be_l[i], dy_done=F.ln_bwd_e, next_ln=self._below("encoder", i, F.ln_bwd_e),
                                   head=head)
            dy = pingpong[n % 2]
        d_x0_e = dy
        if cfg.kind == "token":
            o.embed_bwd(self.tokens, st.grad("encoder.embedding.weight"), d_x0_e.view(B, Se, -1), 0, sq_e,
                        classes=self.classes, dcls=st.grad("encoder.class2hid.weight"))
        else:
            # with cls_fold, rows in_dim.. of this problem are the class table's gradient (model.py:89: one class row per frame)
            self._wgrads.append(o.wgrad_problem(self.roll_cls, d_x0_e, st.grad("encoder.embedding.weight"), M=B * T,
                                                N=cfg.in_dim + (cfg.num_classes if F.cls_fold else 0), K=De, scale=sq_e))
            if not F.cls_fold:
                o.group_colsum(d_x0_e.view(B, Se, -1), T, De, 0, self.classes, st.grad("encoder.class2hid.weight"), sq_e)
        # every (remaining) Dense weight / bias gradient in ONE launch — all 15 problems of the step at configs[1] on a
        # single GPU: one resident round of workgroups with the smallest possible M-split instead of six launches
        self._flush_grads()

    def optimizer(self):
        st = self.store
        deferred = self.forms.shadows != "own"
        sched = st.sched if self.forms.sched else None  # (the launch that carries the bookkeeping reads it)
        clip = self.clip if self.clip is not None else -1.0
        # end-of-step bookkeeping (total loss, running metric sums) on the first Adam launch: losses(combine=False)
        guard = self._guard()
        mt = dict(recon=self.recon, kl=self.kl, kl_weight=self.kl_weight, total=self.total, metric=self.metric_acc, **guard)
        # one launch over the whole bucket, or — two loss scales — one per range: encoder.* tensors come first in the flat buffers,
        # everything from decoder.latent2hid on is decoder-side. NOTE the latent_proj gradients are produced by latent_bwd_vec at the
        # encoder-side scale.
        ranges = [(0, st.n, self.gscale)]
        if self.gscale != self.gscale_enc:
            cut = st.offsets["decoder.latent2hid.weight"]
            ranges = [(0, cut, self.gscale_enc), (cut, st.n, self.gscale)]
        rescale = [1.0 / (self.global_batch * gs) for _, _, gs in ranges]
        if self.forms.gnorm:
            # clipping by the global norm: every Adam launch of the step reads the same sums of squares — taken here, behind the
            # all-reduce, from the whole bucket at the launches' own rescales
            o.grad_sumsq(st.g, ranges[-1][0], rescale[0], rescale[-1], self.grad_parts)
        for (a, b, _), r in zip(ranges, rescale):
            first = a == 0  # the launch that carries the bookkeeping: the metrics, the schedule block, the clipping statistics
            o.adam_flat(st.w[a:b], st.g[a:b], st.m[a:b], st.v[a:b], st.w16[a:b], st.step_state, lr=self.lr, rescale=r, clip=clip,
                        advance_step=False, metrics=mt if first else (guard or None), sched=sched if first else None,
                        emb=dict(base=a, specs=st.emb_specs, wt16=st.wt16) if deferred else None,
                        gnorm=dict(parts=self.grad_parts, max_norm=self.clip_global_norm, gstat=st.gstat if first else None)
                        if self.forms.gnorm else None,
                        # the average: each launch folds the weights of its own range into the same range of store.ema
                        ema=dict(buf=st.ema[a:b], decay=self.ema_decay) if self.forms.ema else None, **self.opt)
        if not deferred:  # (deferred: the next step's first launch rebuilds them, forward())
            o.transpose_shadows(st.w, st.wt16, st.t_desc, st.t_prefix, len(st.t_specs), st.t_tiles)

    # ------------------------------------------------------------------------------ step
    def fwd_bwd_kernels(self, is_train=True):
        self._tick_adam = is_train  # the step counter / lr_t are advanced by forward()'s step_begin launch
        self.forward(with_grad=is_train)
        self.losses(with_grad=is_train, combine=not is_train)
        if is_train:
            self.backward()

    def step_kernels(self, is_train=True, reduce_fn=None):
        """One step, eagerly: forward, losses, backward, [gradient all-reduce], Adam + shadow refresh."""
        self.fwd_bwd_kernels(is_train)
        if is_train:
            if reduce_fn is not None:
                reduce_fn(self.store.g)
            self.optimizer()

    def capture(self, is_train=True, split_optimizer=False, overlap=False):
        """Capture the step into hipGraph(s) on the current stream. Run one eager step of this shape
        first (lazy HIP module loads are not capturable). With split_optimizer the optimizer lives in
        its own graph so a gradient all-reduce can run between the two (data parallel). With overlap as well (and an
        encoder of >= 2 layers) the backward pass is cut after the top encoder layer: run(reducer=...) all-reduces the
        early part of the bucket on the communication stream while the rest of the backward pass executes."""
        self.is_train, self.split = is_train, split_optimizer
        self.graph_late = None
        if is_train and split_optimizer and overlap and self.grad_cut() > 0:
            def early():
                self._tick_adam = True
                self.forward(with_grad=True)
                self.losses(with_grad=True, combine=False)
                self.backward_early(flush=True)
            self.graph = o.Graph().capture(early)
            self.graph_late = o.Graph().capture(self.backward_late)
            self.graph_opt = o.Graph().capture(self.optimizer)
        elif split_optimizer or not is_train:
            self.graph = o.Graph().capture(lambda: self.fwd_bwd_kernels(is_train))
            self.graph_opt = o.Graph().capture(self.optimizer) if is_train else None
        else:
            self.graph = o.Graph().capture(lambda: self.step_kernels(True))
            self.graph_opt = None
        return self

    def graph_nodes(self):
        """(nodes, kernel launches among them) of the captured step, summed over its graphs"""
        gs = [g for g in (self.graph, self.graph_late, self.graph_opt) if g is not None]
        return sum(g.nodes for g in gs), sum(g.kernel_nodes for g in gs)

    def run(self, reduce_fn=None, reducer=None, stamps=None):
        """Replay the captured step. reduce_fn(flat): blocking-in-stream-order all-reduce of the whole bucket between the
        two graphs. reducer (parallel.GradReducer): asynchronous per-range all-reduce, used with capture(overlap=True).
        stamps: a pair of ops.Event recorded on the step's stream behind the last backward graph and in front of the
        optimizer graph — the time between them is the part of the gradient exchange that nothing hides."""
        if self.graph is None:
            raise RuntimeError("call capture() first")
        self.graph.launch()
        g = self.store.g
        if self.graph_late is not None:
            cut = self.grad_cut()
            pending = [reducer.start(g[cut:])] if reducer is not None else []
            self.graph_late.launch()  # runs while the early part of the bucket is on the wire
            self._exchange_and_step(g[:cut], pending, reduce_fn, reducer, stamps)
        elif self.graph_opt is not None:
            self._exchange_and_step(g, [], reduce_fn, reducer, stamps)

    def _exchange_and_step(self, rest, pending, reduce_fn, reducer, stamps):
        """run()'s part between the last backward graph and the optimizer graph: stamp 0, the exchange of the gradient bucket — the
        reducer takes `rest`, the part not yet on the wire, and waits for it and for the `pending` ones; reduce_fn takes the whole
        bucket —, stamp 1, the optimizer graph"""
        if stamps is not None:
            stamps[0].record()
        if reducer is not None:
            reducer.finish(pending + [reducer.start(rest)])
        elif reduce_fn is not None:
            reduce_fn(self.store.g)
        if stamps is not None:
            stamps[1].record()
        self.graph_opt.launch()

    def metrics(self, reset=True):
        """(kl_loss, total_loss) batch means accumulated on the device (trainer.py:115-116,185-186); one sync."""
        m = self.store.read_metrics(reset)
        n = max(m["count"], 1.0)
        return {"kl_loss": m["kl_sum"] / n, "total_loss": m["total_sum"] / n, "count": m["count"], "nonfinite_steps": m["nonfinite_steps"],
                "kl_weight": m.get("kl_weight", self.kl_weight) if self.scheduled else self.kl_weight,
                "lr_scale": m.get("lr_scale", 1.0) if self.scheduled else 1.0,
                **{k: m[k] for k in ("grad_norm", "grad_norm_max", "clip_frac") if k in m}}
