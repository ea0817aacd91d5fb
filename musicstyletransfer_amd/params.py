"""ParamStore: the flat parameter / gradient / Adam-state buffers in HBM, their 16-bit shadows, the running metric sums, and the
per-layer parameter records (Dense, Norm, LayerParams) it hands to the kernels' front end."""
import contextlib
import os
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops as o
from ._lib import CE_MAX_WORKGROUPS, ROLL_SLOTS
from .ops import roundup
from .spec import logical_param_shapes, xavier_init

# Parameter views of one transformer layer as the kernels take them (ParamStore.layer). Dense: w the 16-bit shadow (GEMM B operand), b the
# fp32 bias, t the transposed 16-bit shadow (dgrad B operand), dw / db their views of the gradient bucket; kqv is the layer's K | Q | V
# projection as ONE [3D, D] Dense. Norm: site is the LayerNorm's key in StepPlan._ln_part. What an encoder and a decoder layer differ in
# is data here: ln2 is the layer's LAST LayerNorm (the decoder's ln3); self_resid: the second residual is the feed-forward output itself
# (decoder, transformer.py:199-200: LN3(ff + dropout(ff))) instead of x1 (encoder: LN2(x1 + dropout(ff))); mask_mode: what the backward
# of that last LayerNorm does with the dropout mask (1: a masked copy of dx next to dx, 2: dx * (1 + mask)).
Dense = namedtuple("Dense", "w b t dw db")
Norm = namedtuple("Norm", "gamma beta dgamma dbeta site")
LayerParams = namedtuple("LayerParams", "kqv proj ff1 ff2 ln1 ln2 self_resid mask_mode")


class ParamStore:
    """Flat parameter / gradient / Adam-state buffers and their 16-bit shadows."""

    def __init__(self, cfg, device, act_dtype=torch.bfloat16, params_np=None, seed=1234):
        self.cfg, self.device, self.act_dtype = cfg, device, act_dtype
        shapes = logical_param_shapes(cfg)
        # flat order: per attention block the three K,Q,V weights first (fused [3D,D] GEMM), then their biases
        order = []
        for name in shapes:
            if ".att.W_q." in name or ".att.W_v." in name:
                continue
            if name.endswith(".att.W_k.weight"):
                p = name[: -len("W_k.weight")]
                order += [p + "W_k.weight", p + "W_q.weight", p + "W_v.weight"]
            elif name.endswith(".att.W_k.bias"):
                p = name[: -len("W_k.bias")]
                order += [p + "W_k.bias", p + "W_q.bias", p + "W_v.bias"]
            else:
                order.append(name)
        if cfg.kind == "pianoroll":
            # the class table right behind the input embedding: [in_dim + C, De] is then ONE matrix, and the class-embedding
            # gradient is the last C rows of the embedding's weight-gradient problem (Forms.cls_fold)
            order.remove("encoder.class2hid.weight")
            order.insert(order.index("encoder.embedding.weight") + 1, "encoder.class2hid.weight")
        self.shapes, self.offsets = shapes, OrderedDict()
        off = 0
        for name in order:
            fused_tail = (".att.W_q." in name) or (".att.W_v." in name)
            if not fused_tail:
                off = roundup(off, 8)
            self.offsets[name] = off
            off += int(np.prod(shapes[name]))
        self.n = roundup(off, 8)
        self.n_params = sum(int(np.prod(s)) for s in shapes.values())
        f32 = dict(dtype=torch.float32, device=device)
        self.w = torch.zeros(self.n, **f32)
        self.g = torch.zeros(self.n, **f32)
        self.m = torch.zeros(self.n, **f32)
        self.v = torch.zeros(self.n, **f32)
        self.w16 = torch.zeros(self.n, dtype=act_dtype, device=device)
        self.step_state = torch.zeros(2, dtype=torch.int32, device=device)

        # transposed shadows: (source offset, rows, cols) -> dst [cols, roundup8(rows)]
        self.t_specs = OrderedDict()
        for side, D, L in (("encoder", cfg.e_model, cfg.e_layers), ("decoder", cfg.d_model, cfg.d_layers)):
            for i in range(L):
                p = f"{side}.layer{i}"
                self.t_specs[f"{p}.att.W_kqv"] = (self.offsets[f"{p}.att.W_k.weight"], 3 * D, D)
                self.t_specs[f"{p}.att.W_proj.weight"] = (self.offsets[f"{p}.att.W_proj.weight"], D, D)
                self.t_specs[f"{p}.ff1.weight"] = (self.offsets[f"{p}.ff1.weight"], 4 * D, D)
                self.t_specs[f"{p}.ff2.weight"] = (self.offsets[f"{p}.ff2.weight"], D, 4 * D)
        self.t_specs["decoder.output_layer.weight"] = (self.offsets["decoder.output_layer.weight"], cfg.out_dim, cfg.d_model)
        if cfg.kind == "pianoroll":
            self.t_specs["encoder.embedding.weight"] = (self.offsets["encoder.embedding.weight"], cfg.in_dim, cfg.e_model)
            self.t_specs["decoder.embedding.weight"] = (self.offsets["decoder.embedding.weight"], cfg.out_dim, cfg.d_model)
        doff, self.t_off = 0, OrderedDict()
        for name, (so, r, c) in self.t_specs.items():
            self.t_off[name] = doff
            doff += c * roundup(r, 8)

        def tables(names):
            """(descriptors {source offset, destination offset, rows, cols}, prefix sums of their 32 x 32 tiles) of the named shadows"""
            desc, prefix = [], [0]
            for name in names:
                so, r, c = self.t_specs[name]
                desc += [so, self.t_off[name], r, c]
                prefix.append(prefix[-1] + ((r + 31) // 32) * ((c + 31) // 32))
            return desc, prefix

        desc, prefix = tables(self.t_specs)
        self.wt16 = torch.zeros(max(doff, 8), dtype=act_dtype, device=device)
        self.t_desc = torch.tensor(desc, dtype=torch.int64, device=device)
        self.t_prefix = torch.tensor(prefix, dtype=torch.int64, device=device)
        self.t_tiles = prefix[-1]
        # Deferred shadow refresh (piano-roll ends): the transposed shadows of the matrices only the BACKWARD pass reads are rebuilt by
        # extra workgroups of the NEXT step's first launch (mst_gemm_nt_pair_begin, sh_*) instead of a launch of their own behind the
        # optimizer; the two embedding tables, which that first launch itself reads, are kept current by the optimizer launch
        # (mst_adam_args.emb). Token ends keep the separate launch.
        emb_names = [n for n in ("encoder.embedding.weight", "decoder.embedding.weight") if n in self.t_specs]
        late = [n for n in self.t_specs if n not in emb_names]
        self.shadows_deferred = cfg.kind == "pianoroll" and len(emb_names) == 2 and len(late) > 0
        ldesc, lprefix = tables(late)
        self.t_desc_late = torch.tensor(ldesc or [0, 0, 1, 1], dtype=torch.int64, device=device)
        self.t_prefix_late = torch.tensor(lprefix, dtype=torch.int64, device=device)
        self.t_n_late, self.t_tiles_late = len(late), lprefix[-1]
        self.emb_specs = [(self.t_specs[n][0], self.t_off[n], self.t_specs[n][1], self.t_specs[n][2]) for n in emb_names]
        # the views of every layer's parameters, built once: the flat buffers never move (captured graphs rely on that)
        self._layers = {(side, i): self._layer_params(side, i)
                        for side, n_l in (("encoder", cfg.e_layers), ("decoder", cfg.d_layers)) for i in range(n_l)}

        # shared by every StepPlan of this store (plans run one after the other on one stream): the per-step RNG state
        # — ONE stream of seeds however many (B, T) shapes a run goes through — and the weight-gradient work buffer
        self._rng_state = None
        self._wgrad_scratch = []
        # running metric sums of every step since the last read (trainer.py:107-120,181-186), whatever plan ran it:
        #   metric_acc = [sum kl, sum total, count]; tok_parts = per-workgroup partial rows of the masked token metrics
        #   {sum -log p[label], #arg-max hits, #top-k hits, #valid} accumulated by mst_softmax_ce (token ends)
        # step_status = three int32 words of the step guard (mst_step_metrics), read with the metrics (same device->host copy):
        # {flags, skipped steps} — sticky, set on the device when a one-launch position-0 tail (mst_row_tail_*) could not finish —
        # and the number of steps the optimizer skipped because a loss was not finite (not sticky: the next batch is tried again)
        # sched = the fp32 schedule block {beta_t, tau, f_lr, t} the step's first launch writes for a plan with training schedules
        # (schedule_values; mst_step_begin_args.sched*), read by that step's scheduled launches — and here, with the metrics
        # gstat = the statistics block of global-norm clipping {norm, c, sum of norms, largest norm, steps, clipped steps}, written by
        # the bookkeeping thread of every counted step of a plan with clip_global_norm (mst_adam_args.gstat), read with the metrics
        self._metric_buf = torch.zeros(20, **f32)
        self.metric_acc = self._metric_buf[:3]
        self.step_status = self._metric_buf[4:7].view(torch.int32)
        self.sched = self._metric_buf[8:12]
        self.gstat = self._metric_buf[12:20]
        self._grad_parts = None
        # the exponential moving average of the weights (enable_ema): a second fp32 bucket at w's offsets, kept by the Adam launches of
        # a plan with ema_decay. None for a store that does not average: it allocates what it always did
        self.ema = None
        self.ema_swapped = False      # True while w holds the averaged weights (swap_ema / ema_weights)
        self.nonfinite_steps = 0      # steps skipped for a non-finite loss since the store was made (read_metrics adds them up)
        self.tail_fused = os.environ.get("MST_ROW_TAIL", "1") != "0"  # False: the five-launch form of the position-0 tails
        self.tail_checked = False     # row_tail_selfcheck() ran for this store
        self.tail_policy = os.environ.get("MST_TAIL_FAILURE", "fallback")  # or "raise"
        self.tail_failures = []       # (flags, skipped steps) of every failure seen
        self._tail_listeners = []
        self._rng_state_infer = None
        self.tok_parts = torch.zeros(CE_MAX_WORKGROUPS, 4, **f32) if cfg.kind == "token" else None
        # roll_counts = the piano-roll ends' slots of {tp, pred, pos, cells} the BCE launches add to (mst_bce_args.counts)
        self.roll_counts = torch.zeros(ROLL_SLOTS, 4, dtype=torch.int64, device=device) if cfg.kind == "pianoroll" else None
        # lat_stats = per class and latent dimension {n, sum mu, sum mu^2, sum sigma^2, sum kl_d} (mst_latent_dim_stats; latent_scores)
        self.lat_stats = torch.zeros(cfg.num_classes, 5, cfg.latent_dim, dtype=torch.float64, device=device)
        # class_mmd_acc = {sum of L over the launches whose L was finite, those launches, the others} of mst_class_mmd (class_mmd_score);
        # beside it the launch's per-row terms (one per sample of the largest batch so far: class_mmd_rows) and its ticket word
        self.class_mmd_acc = torch.zeros(3, dtype=torch.float64, device=device)
        self._class_mmd_rows = [torch.zeros(256, dtype=torch.float64, device=device)]
        self.class_mmd_ticket = torch.zeros(1, dtype=torch.int32, device=device)
        if params_np is None:
            params_np = xavier_init(cfg, np.random.default_rng(seed))
        self.load_numpy(params_np)

    def rng_state(self, seed=0):
        """uint64[4] device state of mst_step_begin / mst_rng_advance, created with the first plan's seed"""
        if self._rng_state is None:
            self._rng_state = torch.tensor([0, 0, seed ^ 0x5DEECE66D, 0], dtype=torch.int64, device=self.device)
        return self._rng_state

    def class_mmd_rows(self, B):
        """the fp64 [>= B] buffer of mst_class_mmd's per-row terms; a batch larger than any so far gets a larger one, and none is ever
        freed: captured graphs keep the pointer (call it where a plan is made, never inside a capture)"""
        if self._class_mmd_rows[-1].numel() < B:
            self._class_mmd_rows.append(torch.zeros(B, dtype=torch.float64, device=self.device))
        return self._class_mmd_rows[-1]

    def grad_parts(self):
        """the per-workgroup sums of squares a step's mst_grad_sumsq launch leaves for its Adam launches (global-norm clipping), made
        for the first plan that asks — a store without such a plan allocates what it always did — and never freed: captured graphs
        keep the pointer"""
        if self._grad_parts is None:
            self._grad_parts = torch.zeros(o.grad_sumsq_parts(), dtype=torch.float32, device=self.device)
        return self._grad_parts

    def enable_ema(self):
        """the average, made for the first plan (or trainer) that asks: a copy of w as it is now — at allocation time, never inside a
        capture — and never freed or moved: captured graphs keep the pointer"""
        if self.ema is None:
            self.ema = self.w.clone()
        return self.ema

    def swap_ema(self):
        """exchange the contents of w and ema in one launch (mst_ema_swap, which also writes w16 from the new w), then the shadow
        refresh, so that every kernel consumes what a store loaded with those weights would. Contents move, pointers do not: every
        captured graph stays valid. Exact: a second call puts back every bit."""
        if self.ema is None:
            raise RuntimeError("this store keeps no average of its weights (StepPlan(ema_decay=...) / enable_ema())")
        o.ema_swap(self.w, self.ema, self.w16)
        self.refresh_shadows()
        self.ema_swapped = not self.ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """with store.ema_weights(): ... — the averaged weights swapped in for validation, sampling or a forward pass, and the raw
        iterate back on exit (also after an exception). No training step may run inside: it would update the average as the weights."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def rng_state_inference(self):
        """the RNG state inference-mode forward passes advance (eps of Model.__call__ when none is given): never the
        training stream's, so that a sampling hook in the middle of training leaves the steps after it as they were"""
        if self._rng_state_infer is None:
            self._rng_state_infer = torch.tensor([0, 0, 0x1F123BB5 ^ 0x5DEECE66D, 0], dtype=torch.int64, device=self.device)
        return self._rng_state_infer

    def on_tail_failure(self, callback):
        """callback() after a failed position-0 tail made this store fall back to the five-launch form: holders of captured
        graphs must drop them (they were recorded with the one-launch kernels)"""
        self._tail_listeners.append(callback)

    def handle_step_status(self, flags, skipped):
        """A one-launch position-0 tail could not do its work in `skipped` steps since the last read (flags: _lib.TAIL_* /
        STEP_INCOMPLETE). The optimizer launches of those steps left the model untouched (step guard), so nothing wrong was
        learned; from here on the five-launch form runs (policy 'fallback'), or the run stops (policy 'raise')."""
        o.zero(self._metric_buf[4:6])
        self.tail_failures.append((int(flags), int(skipped)))
        self.tail_fused = False
        msg = (f"the one-launch position-0 tail of the top encoder layer failed (status flags {int(flags):#x}: "
               f"{'forward barrier timed out; ' if flags & 1 else ''}{'backward barrier timed out; ' if flags & 2 else ''}"
               f"{'tail incomplete at the end of a step; ' if flags & 16 else ''}"
               f"{int(skipped)} step(s) skipped without touching the model)")
        if self.tail_policy == "raise":
            raise RuntimeError(msg + " — MST_TAIL_FAILURE=raise")
        warnings.warn(msg + "; falling back to the five-launch form for the rest of the run", RuntimeWarning)
        for cb in self._tail_listeners:
            cb()

    def poll_status(self, reduce=None):
        """Cheap, NON-BLOCKING look at the step guard's sticky words, for the training loop to call every few steps (the
        words are otherwise read only with the metrics — at the periodic log — and after one failed tail every following
        step is a skipped batch until then). Two halves per call, no synchronisation in either: (1) if the copy the previous
        call started has arrived (event query), look at it: a set flag goes to handle_step_status() — fall back to the
        five-launch form at once, or raise; (2) start the next asynchronous copy of the words into page-locked memory
        behind everything launched so far on the current stream. reduce(tensor): data parallel — an in-place SUM over the
        ranks applied to a float copy of the words first, so that every rank sees a failure of ANY rank at the same poll
        and all of them stop together (handle_step_status raises there: a skipped update on one rank lets the replicas drift).
        Returns True when a failure was handled."""
        if getattr(self, "_poll_host", None) is None:
            self._poll_host = torch.zeros(2, dtype=torch.float32).pin_memory()
            self._poll_dev = torch.zeros(2, dtype=torch.float32, device=self.device)
            self._poll_event = torch.cuda.Event()
            self._poll_pending = False
        handled = False
        if self._poll_pending and self._poll_event.query():
            self._poll_pending = False
            flags, skipped = (int(v) for v in self._poll_host.tolist())
            if flags or skipped:
                if reduce is not None:  # (summed over the ranks: only "non-zero" means anything)
                    self.tail_fused = False
                    raise RuntimeError(f"a one-launch position-0 tail failed on at least one rank (status words summed over the ranks: "
                                       f"{flags}, {skipped} skipped step(s)); the replicas are no longer identical — restart from the "
                                       "last checkpoint with MST_ROW_TAIL=0")
                cur = self.step_status[:2].tolist()  # (one small blocking read, on the failure path only: the words as they are NOW)
                self.handle_step_status(cur[0] or flags, cur[1] or skipped)
                handled = True
        if not self._poll_pending:
            self._poll_dev.copy_(self.step_status[:2])
            if reduce is not None:
                reduce(self._poll_dev)
            self._poll_host.copy_(self._poll_dev, non_blocking=True)
            self._poll_event.record()
            self._poll_pending = True
        return handled

    def read_metrics(self, reset=True):
        """one device->host read of the running sums: {'kl_sum', 'total_sum', 'count'} and, for the token ends,
        {'nll_sum', 'acc_hits', 'topk_hits', 'n_tokens'}, for the piano-roll ends the counts {'roll_tp', 'roll_pred', 'roll_pos',
        'roll_cells'} as ints (roll_scores turns them into precision / recall / F1) (the caller orders this after the steps it wants included).
        The step-status words travel in the same copy: a set flag is handled here (handle_step_status). So does the schedule
        block: once a plan with training schedules has run, 'kl_weight' (beta_t) and 'lr_scale' (f_lr) of the last such step.
        (The last step that RAN: after a step the guards skipped, whose step count was taken back, the block still holds that
        step's values until the next step's first launch writes it again from the count — training is unaffected.)
        And the statistics of global-norm clipping: once a step of a plan with clip_global_norm has counted, 'grad_norm' (the mean
        norm before clipping over the counted steps since the last reset), 'grad_norm_max' and 'clip_frac' (the share of them that
        were clipped); reset clears these running fields with the sums."""
        buf = self._metric_buf.cpu()
        acc = buf[:3].tolist()
        flags, skipped, nonfinite = buf[4:7].view(torch.int32).tolist()
        if nonfinite:
            # (the optimizer left the model alone in those steps: an overflowed activation or sigma = 0 would have made every
            # gradient NaN — mst_step_metrics' non-finite guard)
            self.nonfinite_steps += int(nonfinite)
            o.zero(self._metric_buf[6:7])
            warnings.warn(f"{int(nonfinite)} training step(s) skipped: a per-sample loss was not finite (an fp16 activation overflow or "
                          "sigma = 0 under log(sigma^2)); parameters, moments and the step count were left as they were", RuntimeWarning)
        if flags or skipped:
            self.handle_step_status(flags, skipped)
        out = {"kl_sum": acc[0], "total_sum": acc[1], "count": acc[2], "skipped_steps": skipped, "nonfinite_steps": int(nonfinite)}
        beta_t, _, f_lr, sched_t = buf[8:12].tolist()
        if sched_t > 0:  # (a scheduled step wrote the block)
            out.update(kl_weight=beta_t, lr_scale=f_lr)
        _, _, norm_sum, norm_max, g_steps, g_clipped = buf[12:18].tolist()
        if g_steps > 0:  # (a step with global-norm clipping counted)
            out.update(grad_norm=norm_sum / g_steps, grad_norm_max=norm_max, clip_frac=g_clipped / g_steps)
        if self.tok_parts is not None:
            t = self.tok_parts.cpu().double().sum(0).tolist()
            out.update(nll_sum=t[0], acc_hits=t[1], topk_hits=t[2], n_tokens=t[3])
        if self.roll_counts is not None:
            c = self.roll_counts.cpu().sum(0).tolist()
            out.update(roll_tp=int(c[0]), roll_pred=int(c[1]), roll_pos=int(c[2]), roll_cells=int(c[3]))
        out["lat_stats"] = self.lat_stats.cpu().numpy()  # (all zero unless a plan with track_latent_stats ran; latent_scores)
        out["class_mmd_acc"] = self.class_mmd_acc.cpu().numpy()  # (all zero unless a plan with class_mmd > 0 ran; class_mmd_score)
        if reset:
            o.zero(self.lat_stats)
            o.zero(self.class_mmd_acc)
            o.zero(self.metric_acc)
            if g_steps > 0:
                o.zero(self.gstat[2:6])
            if self.tok_parts is not None:
                o.zero(self.tok_parts)
            if self.roll_counts is not None:
                o.zero(self.roll_counts)
        return out

    def wgrad_scratch(self, n_floats=16 * 1024 * 1024 + 256 * 256):
        """fp32 work buffer of the wgrad launch's two-pass reduction: one full resident round of 256 x 256 slab tiles
        (256 work items x 256 KiB = 64 MiB) plus each item's 256 bias column sums (256 KiB) is all
        mst_gemm_wgrad_batch_flush ever asks for. Buffers are never freed:
        captured graphs keep the pointer they were recorded with."""
        for t in self._wgrad_scratch:
            if t.numel() >= n_floats:
                return t
        t = torch.empty(n_floats, dtype=torch.float32, device=self.device)
        self._wgrad_scratch.append(t)
        return t

    # ---- views
    def _view(self, flat, name):
        shape = self.shapes[name]
        off = self.offsets[name]
        return flat[off: off + int(np.prod(shape))].view(*shape)

    def p(self, name):
        return self._view(self.w, name)

    def grad(self, name):
        return self._view(self.g, name)

    def h(self, name):
        return self._view(self.w16, name)

    def fused(self, flat, prefix, what):
        """[3D, D] weight or [3D] bias view of a layer's K,Q,V Dense layers (K rows first)"""
        D = self.shapes[f"{prefix}.att.W_k.weight"][0]
        off = self.offsets[f"{prefix}.att.W_k.{what}"]
        return flat[off: off + 3 * D * D].view(3 * D, D) if what == "weight" else flat[off: off + 3 * D]

    def t(self, name):
        so, r, c = self.t_specs[name]
        off = self.t_off[name]
        return self.wt16[off: off + c * roundup(r, 8)].view(c, roundup(r, 8))

    def _layer_params(self, side, i):
        pre = f"{side}.layer{i}"

        def dense(name):
            w, b = f"{pre}.{name}.weight", f"{pre}.{name}.bias"
            return Dense(self.h(w), self.p(b), self.t(w), self.grad(w), self.grad(b))

        def norm(name):
            g, b = f"{pre}.{name}.gamma", f"{pre}.{name}.beta"
            return Norm(self.p(g), self.p(b), self.grad(g), self.grad(b), f"{pre}.{name}")

        kqv = Dense(self.fused(self.w16, pre, "weight"), self.fused(self.w, pre, "bias"), self.t(f"{pre}.att.W_kqv"),
                    self.fused(self.g, pre, "weight"), self.fused(self.g, pre, "bias"))
        dec = side == "decoder"
        return LayerParams(kqv, dense("att.W_proj"), dense("ff1"), dense("ff2"), norm("ln1"), norm("ln3" if dec else "ln2"),
                           self_resid=dec, mask_mode=2 if dec else 1)

    def layer(self, side, i):
        """the LayerParams record of layer i of the 'encoder' / 'decoder' stack"""
        return self._layers[side, i]

    # ---- host <-> device
    def _flatten(self, params_np):
        """name -> array as one host bucket in the flat buffers' layout"""
        host = np.zeros(self.n, np.float32)
        for name, shape in self.shapes.items():
            a = np.asarray(params_np[name], np.float32)
            assert tuple(a.shape) == tuple(shape), f"{name}: expected {shape}, got {a.shape}"
            host[self.offsets[name]: self.offsets[name] + a.size] = a.reshape(-1)
        return torch.from_numpy(host)

    def load_numpy(self, params_np):
        self.w.copy_(self._flatten(params_np))
        self.refresh_shadows()

    def to_numpy(self, which="w"):
        """name -> host copy of the tensor's part of a flat fp32 bucket: 'w', 'g', 'm', 'v', or 'ema' (a store that averages)"""
        if which == "ema" and self.ema is None:
            raise RuntimeError("this store keeps no average of its weights (StepPlan(ema_decay=...) / enable_ema())")
        host = getattr(self, which).detach().cpu().numpy()
        return OrderedDict((n, host[self.offsets[n]: self.offsets[n] + int(np.prod(s))].reshape(s).copy())
                           for n, s in self.shapes.items())

    def shadowed_names(self):
        """parameters the kernels consume through a 16-bit shadow (GEMM B operands); every other tensor — biases,
        LayerNorm gamma / beta, class tables, the latent block, token embedding tables — is read in fp32"""
        names = set()
        for key in self.t_specs:
            if key.endswith(".att.W_kqv"):
                p = key[: -len("W_kqv")]
                names.update({p + "W_k.weight", p + "W_q.weight", p + "W_v.weight"})
            else:
                names.add(key)
        return names

    def as_consumed_numpy(self):
        """name -> the values the kernels actually read: the 16-bit shadow (widened to fp32) for shadowed_names(), the
        fp32 master otherwise. Feeding these to a reference separates weight rounding from kernel error."""
        w = self.to_numpy("w")
        w16 = self.w16.detach().float().cpu().numpy()
        for n in self.shadowed_names():
            s = self.shapes[n]
            w[n] = w16[self.offsets[n]: self.offsets[n] + int(np.prod(s))].reshape(s).copy()
        return w

    def load_ema_numpy(self, params_np=None):
        """set the average from name -> array (a checkpoint's), or to a copy of w (None)"""
        self.enable_ema()
        if params_np is None:
            self.ema.copy_(self.w)
            return
        self.ema.copy_(self._flatten(params_np))

    def refresh_shadows(self):
        o.cast_to_act(self.w, self.w16)
        o.transpose_shadows(self.w, self.wt16, self.t_desc, self.t_prefix, len(self.t_specs), self.t_tiles)
