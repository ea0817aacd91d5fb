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
import contextlib
import math
import os
import warnings
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops as o
from ._lib import CE_MAX_WORKGROUPS, ROLL_SLOTS
from .ops import roundup


class VAEConfig:
    """Shape of the model: the union of ModelConfig/EncoderConfig/DecoderConfig/TransformerConfig
    (model.py:22-54, transformer.py:8-21) flattened, plus which ends are attached:
    kind='token' (Embedding in, softmax-CE out: the reference's executed path) or
    kind='pianoroll' (multi-hot frame x table in, sigmoid + BinaryCrossEntropy out)."""

    def __init__(self, kind, in_dim, out_dim, num_classes, latent_dim, e_model, e_layers, e_heads, d_model, d_layers,
                 d_heads, e_dropout=0.0, d_dropout=0.0, d_causal=False):
        assert kind in ("token", "pianoroll")
        assert e_model % e_heads == 0 and d_model % d_heads == 0  # transformer.py:134,167
        self.kind = kind
        self.in_dim, self.out_dim = in_dim, out_dim
        self.num_classes, self.latent_dim = num_classes, latent_dim
        self.e_model, self.e_layers, self.e_heads = e_model, e_layers, e_heads
        self.d_model, self.d_layers, self.d_heads = d_model, d_layers, d_heads
        self.e_dropout, self.d_dropout = float(e_dropout), float(d_dropout)
        # d_causal: the decoder's self-attention is causal with a softmax over the keys (mst_attn_causal_fwd/bwd), the model
        # DecodePlan(attention="key") samples from. Off: the reference's non-causal query-axis softmax (transformer.py:174,100).
        self.d_causal = bool(d_causal)

    def as_dict(self):
        return dict(self.__dict__)


def positional_table(model_size, max_len):
    """transformer.py:204-211: exponent 2*i/D for every column, sin on even / cos on odd columns,
    float64 then cast (host-side constant, built once)."""
    pos = np.arange(max_len).reshape((-1, 1)) / np.power(10000, (2.0 / model_size) * np.arange(model_size).reshape((1, -1)))
    pos[:, 0::2] = np.sin(pos[:, 0::2])
    pos[:, 1::2] = np.cos(pos[:, 1::2])
    return pos.astype(np.float32)


def logical_param_shapes(cfg):
    """name -> shape in the reference's construction order (model.py:57-71,206-227;
    transformer.py:24-46,49-68,129-149,162-182): 58 tensors at e_layers=2, d_layers=1."""
    s = OrderedDict()
    De, Dd, Z, C = cfg.e_model, cfg.d_model, cfg.latent_dim, cfg.num_classes

    def layer(prefix, D, last_ln):
        for w in ("W_k", "W_q", "W_v", "W_proj"):
            s[f"{prefix}.att.{w}.weight"] = (D, D)
            s[f"{prefix}.att.{w}.bias"] = (D,)
        s[f"{prefix}.ln1.gamma"] = (D,)
        s[f"{prefix}.ln1.beta"] = (D,)
        s[f"{prefix}.ff1.weight"] = (4 * D, D)
        s[f"{prefix}.ff1.bias"] = (4 * D,)
        s[f"{prefix}.ff2.weight"] = (D, 4 * D)
        s[f"{prefix}.ff2.bias"] = (D,)
        s[f"{prefix}.{last_ln}.gamma"] = (D,)
        s[f"{prefix}.{last_ln}.beta"] = (D,)

    s["encoder.class2hid.weight"] = (C, De)
    s["encoder.embedding.weight"] = (cfg.in_dim, De)
    for i in range(cfg.e_layers):
        layer(f"encoder.layer{i}", De, "ln2")
    s["encoder.latent_proj.weight"] = (2 * Z, De)
    s["encoder.latent_proj.bias"] = (2 * Z,)
    s["decoder.latent2hid.weight"] = (Dd, Z)
    s["decoder.latent2hid.bias"] = (Dd,)
    s["decoder.class2hid.weight"] = (C, Dd)
    s["decoder.embedding.weight"] = (cfg.out_dim, Dd)
    for i in range(cfg.d_layers):
        layer(f"decoder.layer{i}", Dd, "ln3")
    s["decoder.output_layer.weight"] = (cfg.out_dim, Dd)
    s["decoder.output_layer.bias"] = (cfg.out_dim,)
    return s


def xavier_init(cfg, rng):
    """trainer.py:103-105 model.initialize(mx.init.Xavier()): uniform, factor 'avg', magnitude 3 for
    every '*weight' (Embedding tables included); biases / beta 0; gamma 1."""
    out = OrderedDict()
    for name, shape in logical_param_shapes(cfg).items():
        if name.endswith("weight"):
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            scale = math.sqrt(3.0 / ((fan_in + fan_out) / 2.0))
            out[name] = rng.uniform(-scale, scale, size=shape).astype(np.float32)
        elif name.endswith("gamma"):
            out[name] = np.ones(shape, np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


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
        desc, prefix, doff, self.t_off = [], [0], 0, OrderedDict()
        for name, (so, r, c) in self.t_specs.items():
            self.t_off[name] = doff
            desc += [so, doff, r, c]
            doff += c * roundup(r, 8)
            prefix.append(prefix[-1] + ((r + 31) // 32) * ((c + 31) // 32))
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
        ldesc, lprefix = [], [0]
        for name in late:
            so, r, c = self.t_specs[name]
            ldesc += [so, self.t_off[name], r, c]
            lprefix.append(lprefix[-1] + ((r + 31) // 32) * ((c + 31) // 32))
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
        if params_np is None:
            params_np = xavier_init(cfg, np.random.default_rng(seed))
        self.load_numpy(params_np)

    def rng_state(self, seed=0):
        """uint64[4] device state of mst_step_begin / mst_rng_advance, created with the first plan's seed"""
        if self._rng_state is None:
            self._rng_state = torch.tensor([0, 0, seed ^ 0x5DEECE66D, 0], dtype=torch.int64, device=self.device)
        return self._rng_state

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
        if reset:
            o.zero(self.lat_stats)
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
    def load_numpy(self, params_np):
        host = np.zeros(self.n, np.float32)
        for name, shape in self.shapes.items():
            a = np.asarray(params_np[name], np.float32)
            assert tuple(a.shape) == tuple(shape), f"{name}: expected {shape}, got {a.shape}"
            host[self.offsets[name]: self.offsets[name] + a.size] = a.reshape(-1)
        self.w.copy_(torch.from_numpy(host))
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
        host = np.zeros(self.n, np.float32)
        for name, shape in self.shapes.items():
            a = np.asarray(params_np[name], np.float32)
            assert tuple(a.shape) == tuple(shape), f"{name}: expected {shape}, got {a.shape}"
            host[self.offsets[name]: self.offsets[name] + a.size] = a.reshape(-1)
        self.ema.copy_(torch.from_numpy(host))

    def refresh_shadows(self):
        o.cast_to_act(self.w, self.w16)
        o.transpose_shadows(self.w, self.wt16, self.t_desc, self.t_prefix, len(self.t_specs), self.t_tiles)


class _Layer:
    pass


# Parameter views of one transformer layer as the kernels take them (ParamStore.layer). Dense: w the 16-bit shadow (GEMM B operand), b the
# fp32 bias, t the transposed 16-bit shadow (dgrad B operand), dw / db their views of the gradient bucket; kqv is the layer's K | Q | V
# projection as ONE [3D, D] Dense. Norm: site is the LayerNorm's key in StepPlan._ln_part. What an encoder and a decoder layer differ in
# is data here: ln2 is the layer's LAST LayerNorm (the decoder's ln3); self_resid: the second residual is the feed-forward output itself
# (decoder, transformer.py:199-200: LN3(ff + dropout(ff))) instead of x1 (encoder: LN2(x1 + dropout(ff))); mask_mode: what the backward
# of that last LayerNorm does with the dropout mask (1: a masked copy of dx next to dx, 2: dx * (1 + mask)).
Dense = namedtuple("Dense", "w b t dw db")
Norm = namedtuple("Norm", "gamma beta dgamma dbeta site")
LayerParams = namedtuple("LayerParams", "kqv proj ff1 ff2 ln1 ln2 self_resid mask_mode")

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
    of an oversubscribed launch landing on one XCD, L1 behaviour of write-through lines — csrc/row_tail.hip), so shape alone does not
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


def roll_scores(tp, pred, pos, cells):
    """the piano-roll counts of ParamStore.read_metrics (a cell is predicted where its logit is > 0) as scores: precision = tp / pred,
    recall = tp / pos, f1 = 2 tp / (pred + pos), cell_acc = (cells - pred - pos + 2 tp) / cells; NaN where a denominator is 0"""
    nan = float("nan")
    return dict(precision=tp / pred if pred else nan, recall=tp / pos if pos else nan,
                f1=2 * tp / (pred + pos) if pred + pos else nan,
                cell_acc=(cells - pred - pos + 2 * tp) / cells if cells else nan)


def latent_scores(acc, threshold=0.01):
    """the per-class, per-dimension sums of ParamStore.read_metrics' 'lat_stats' (fp64 [C, 5, Z], planes {n, sum mu, sum mu^2,
    sum sigma^2, sum kl_d}: mst_latent_dim_stats) as scores. Per dimension d, pooled over the classes: n, m = sum mu / n,
    V = sum mu^2 / n - m^2 (the variance of the posterior mean over the data).
      active_units  number of dimensions with V > threshold (Burda et al.'s 0.01)
      kl_dims       [Z] mean KL of each dimension, sum kl_d / n
      kl_dim_max    the largest of kl_dims
      kl_dims_used  number of dimensions with mean KL > threshold
      sigma_rms     sqrt(mean over d of sum sigma^2 / n)
      class_leak    max over the active dimensions of eta^2_d = sum_c (n_c / n) (m_cd - m_d)^2 / V_d, the share of a dimension's variance
                    that lies BETWEEN the classes (0: z says nothing about the class; 1: the class alone decides mu_d). NaN without an
                    active dimension, or when fewer than two classes have samples.
    A dimension with n == 0 has NaN entries and is not active (kl_dim_max and sigma_rms are taken over the dimensions with samples)."""
    acc = np.asarray(acc, np.float64)
    if acc.ndim != 3 or acc.shape[1] != 5:
        raise ValueError(f"latent_scores takes [C, 5, Z] sums, not {acc.shape}")
    nan = float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        n_c = acc[:, 0]                                   # [C, Z]
        n, s_mu, s_mu2, s_s2, s_kl = acc.sum(0)           # [Z] each
        m = s_mu / n
        var = s_mu2 / n - m * m
        kl_dims = s_kl / n
        active = var > threshold                          # (NaN compares false)
        m_c = acc[:, 1] / n_c                             # [C, Z]; NaN for a class without samples: its weight below is 0
        between = np.where(n_c > 0, n_c / n * (m_c - m) ** 2, 0.0).sum(0)
        eta2 = np.minimum(between / var, 1.0)             # (between <= V; the two are rounded apart)
    seen = n > 0
    classes_seen = int((n_c.sum(1) > 0).sum())
    leak = float(eta2[active].max()) if active.any() and classes_seen >= 2 else nan
    return dict(active_units=int(active.sum()), kl_dims=kl_dims, kl_dim_max=float(kl_dims[seen].max()) if seen.any() else nan,
                kl_dims_used=int((kl_dims > threshold).sum()),
                sigma_rms=float(np.sqrt((s_s2[seen] / n[seen]).mean())) if seen.any() else nan, class_leak=leak)


def iw_scores(acc, cells):
    """the six running sums of IWBound (ops.IW_ACC: sum log_px, sum elbo, sum ess, sum n, pieces counted, pieces invalid — mst_iw_finish)
    as the reported figures, stated once. cells: cells per piece (T * P for a piano-roll, T for a token sequence). Nats per piece:
      iw_nll            -sum log_px / pieces     the importance-weighted bound on -log p(x)
      iw_elbo_nll       -sum elbo / pieces       the same draws' mean log-weight: the ELBO in nats
      iw_gap            iw_elbo_nll - iw_nll     >= 0 (Jensen); near 0: the posterior is tight, or the decoder ignores z
      iw_ess            sum ess / pieces         effective sample size of the weights, between 1 and K
      iw_bits_per_cell  iw_nll / (cells ln 2)
      iw_invalid        pieces with a draw that was not finite (in none of the sums)
    NaN where no piece was counted."""
    acc = np.asarray(acc, np.float64).reshape(-1)
    if acc.size != 6:
        raise ValueError(f"iw_scores takes the six sums of mst_iw_finish, not {acc.size} values")
    if not cells > 0:
        raise ValueError(f"cells per piece must be positive, not {cells!r}")
    pieces, nan = acc[4], float("nan")
    nll = -acc[0] / pieces if pieces > 0 else nan
    elbo_nll = -acc[1] / pieces if pieces > 0 else nan
    return dict(iw_nll=float(nll), iw_elbo_nll=float(elbo_nll), iw_gap=float(elbo_nll - nll),
                iw_ess=float(acc[2] / pieces) if pieces > 0 else nan, iw_bits_per_cell=float(nll / (cells * math.log(2.0))),
                iw_invalid=int(acc[5]))


def check_iw(samples):
    """samples: K of the importance-weighted bound, an integer >= 1 (1: the one-sample ELBO); raises ValueError otherwise (a NaN, a
    bool and a fraction too)"""
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError(f"iw_samples must be an integer >= 1, not {samples!r}")


def check_schedule(kl_warmup_steps=0, kl_cycle_steps=0, kl_free_bits=0.0, lr_warmup_steps=0):
    """the combinations of training-schedule settings that mean something; raises ValueError otherwise"""
    for name, val in (("kl_warmup_steps", kl_warmup_steps), ("kl_cycle_steps", kl_cycle_steps), ("lr_warmup_steps", lr_warmup_steps)):
        if int(val) != val or val < 0:
            raise ValueError(f"{name} must be a non-negative integer, not {val!r}")
    if not kl_free_bits >= 0:
        raise ValueError(f"kl_free_bits must be >= 0 nats per sample, not {kl_free_bits!r}")
    if kl_cycle_steps > 0 and kl_warmup_steps == 0:
        raise ValueError("kl_cycle_steps restarts the KL warm-up: it needs kl_warmup_steps > 0")
    if kl_cycle_steps > 0 and kl_warmup_steps > kl_cycle_steps:
        raise ValueError(f"kl_warmup_steps ({kl_warmup_steps}) must not exceed kl_cycle_steps ({kl_cycle_steps})")


def check_clip(clip_global_norm=0.0):
    """clip_global_norm: 0 (off) or a positive finite bound on the gradient's global L2 norm; raises ValueError otherwise"""
    if not (0 <= clip_global_norm < float("inf")):
        raise ValueError(f"clip_global_norm must be 0 (off) or a positive finite norm, not {clip_global_norm!r}")


def check_input_dropout(d_input_dropout=0.0):
    """d_input_dropout: probability in [0, 1] that a decoder input position is dropped in a training step (0: off, 1: every position);
    raises ValueError otherwise (a NaN too)"""
    if not (0 <= d_input_dropout <= 1):
        raise ValueError(f"d_input_dropout must lie in [0, 1], not {d_input_dropout!r}")


def clip_scale(norm, max_norm):
    """the factor c global-norm clipping applies to a gradient of L2 norm `norm` — gluon.utils.clip_global_norm's rule as the device
    evaluates it (mst_adam_flat's clipping group), stated once for the host in np.float32 arithmetic: c = max_norm / (norm + 1e-8), and 1 unless
    that is below 1"""
    c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-8))
    return c if c < np.float32(1) else np.float32(1)


def check_ema(ema_decay=0.0):
    """ema_decay: 0 (off) or the decay of the weights' exponential moving average, in (0, 1); raises ValueError otherwise (a NaN too)"""
    if not (0 <= ema_decay < 1):
        raise ValueError(f"ema_decay must be 0 (off) or lie in (0, 1), not {ema_decay!r}")


def ema_decay_at(t, decay):
    """d_t, the decay the average applies at training step t (Adam's step count after the step's increment, 1-based) — the rule as the
    device evaluates it (mst_adam_flat's averaging group), stated once for the host in np.float32 arithmetic: min(decay, (1 + t) / (10 + t)), the usual
    warm-up, so that the first steps do not average in the initial weights"""
    tf = np.float32(t)
    d = (np.float32(1) + tf) / (np.float32(10) + tf)
    return min(np.float32(decay), d)


def ema_update(e, w_new, d):
    """the average after a step: fl(fl(d * e) + fl((1 - d) * w_new)) in np.float32 — two rounded products and one rounded sum, in this
    order and never fused, which is what mst_adam_flat computes for mst_adam_args.ema (include/mst_hip.h) bit for bit. e, w_new: fp32 arrays (or scalars)"""
    d = np.float32(d)
    omd = np.float32(1) - d
    a = d * np.asarray(e, np.float32)
    b = omd * np.asarray(w_new, np.float32)
    return a + b


def schedule_values(t, kl_weight=1.0, kl_warmup_steps=0, kl_cycle_steps=0, lr_warmup_steps=0):
    """(beta_t, f_lr) of training step t (Adam's step count after the step's increment, 1-based) — the formulas the device evaluates
    (step_begin.hpp), stated once for the host. Double arithmetic; beta_t is rounded once, to fp32, and returned as that value:
        f_lr   = min(1, t / W_lr) if W_lr > 0 else 1                 the step runs at lr * f_lr
        u      = ((t - 1) mod C) + 1 if C > 0 else t                 position in the current KL cycle
        beta_t = fp32(fp32(kl_weight) * (min(1, u / W_b) if W_b > 0 else 1))"""
    f_lr = min(1.0, t / lr_warmup_steps) if lr_warmup_steps > 0 else 1.0
    u = (t - 1) % kl_cycle_steps + 1 if kl_cycle_steps > 0 else t
    ramp = min(1.0, u / kl_warmup_steps) if kl_warmup_steps > 0 else 1.0
    return float(np.float32(float(np.float32(kl_weight)) * ramp)), f_lr


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
        self._tick_adam = False
        self._infer = False
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
        handed = None
        if next_ln is not None:  # the layer below starts its backward pass with a LayerNorm backward: run it here
            kw, t_below = next_ln
            o.gemm_nt_ln_bwd(t.dqkv, P.kqv.t, t_below.dh, N=D, K=3 * D, resid=t.dh1, **kw)
        elif side == "encoder" and i > 0 and F.kqv_head_e:  # the layer below forms it in front of its leading LayerNorm backward
            handed = dict(A=t.dqkv, B=P.kqv.t, resid=t.dh1, N=D, K=3 * D)
        elif ride:
            T_ = self.T
            handed = (dict(A=t.dqkv, B=P.kqv.t, C_out=dx_in, M=self.B * T_, N=D, K=3 * D, resid=t.dh1, resid_phys=True,
                           a_remap=(T_, T_ + 1, 1), c_remap=(T_, T_ + 1, 1)),
                      (t.dqkv.view(self.B, S, -1), P.kqv.t, t.dh1.view(self.B, S, -1)))
        else:
            o.gemm_nt(t.dqkv, P.kqv.t, dx_in, N=D, K=3 * D, resid=t.dh1)
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
        self._kqv_head = None
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
        if next_ln is not None:  # as in _layer_bwd: the layer below's LayerNorm-2 backward rides on this GEMM
            kw, t_below = next_ln
            o.gemm_nt_ln_bwd(c.dqkv, P.kqv.t, t_below.dh, N=D, K=3 * D, resid=c.dh1, **kw)
        elif i > 0 and F.kqv_head_e:  # as in _layer_bwd: left to the one-launch block of the layer below (the first launch of backward_late)
            self._kqv_head = dict(A=c.dqkv, B=P.kqv.t, resid=c.dh1, N=D, K=3 * D)
        else:
            o.gemm_nt(c.dqkv, P.kqv.t, dx_in, N=D, K=3 * D, resid=c.dh1)
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
        if self.graph_late is not None:
            g, cut = self.store.g, self.grad_cut()
            pending = [reducer.start(g[cut:])] if reducer is not None else []
            self.graph_late.launch()  # runs while the early part of the bucket is on the wire
            if stamps is not None:
                stamps[0].record()
            if reducer is not None:
                pending.append(reducer.start(g[:cut]))
                reducer.finish(pending)
            elif reduce_fn is not None:
                reduce_fn(g)
            if stamps is not None:
                stamps[1].record()
            self.graph_opt.launch()
            return
        if self.graph_opt is not None:
            if stamps is not None:
                stamps[0].record()
            if reducer is not None:
                reducer.finish([reducer.start(self.store.g)])
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


class IWBound:
    """The importance-weighted bound on log p(x) of the batch in `plan`'s input buffers from K posterior draws (Burda et al.):
    log p(x) ~= log (1/K) sum_k p(x | z_k) p(z_k) / q(z_k | x), folded on the device (mst_iw_fold / mst_iw_finish).

    run(K): state is zeroed; ONE full inference forward encodes the batch and is draw 1; draws 2..K are draw passes
    (StepPlan.forward(inference=True, start="latent")): the decoder half alone, from one captured graph that is replayed — the draws
    differ between replays because the seed lives on the device (the store's INFERENCE stream: the training stream is left alone).
    Every draw is scored with the plain likelihood (StepPlan.losses(plain=True)) and folded; mst_iw_finish then writes the per-piece
    rows into `out` and ADDS the batch's sums to `acc`, which several runners may share (the trainer's validation set: one read).

    plan: a StepPlan with internal_eps (eps is drawn per global sample index, plan.sample_offset: a data-parallel shard draws what
    the whole batch draws for its samples). The first draw pass of a runner is issued eagerly (HIP modules load lazily and are not
    capturable), the graph is captured once and kept while the plan's launch forms and bound input blob stay what they were.
    keep_draws=True (tests, small shapes): every draw's eps, sigma, z, recon and seed are copied to [K, ...] buffers (self.draws);
    that path issues every draw eagerly."""

    def __init__(self, plan, acc=None):
        if not plan.internal_eps:
            raise ValueError("IWBound needs a plan that draws its own eps (StepPlan(internal_eps=True))")
        cfg, dev = plan.cfg, plan.dev
        self.plan = plan
        self.cells = plan.T * (cfg.out_dim if cfg.kind == "pianoroll" else 1)  # what the mean reconstruction loss was taken over
        self.recon_scale = float(self.cells)
        f64 = dict(dtype=torch.float64, device=dev)
        self.state = torch.zeros(plan.B, len(o.IW_STATE), **f64)
        self.out = torch.zeros(plan.B, len(o.IW_OUT), **f64)
        self.acc = acc if acc is not None else torch.zeros(len(o.IW_ACC), **f64)
        self.graph, self._graph_key = None, None
        self.captures = 0       # graphs captured so far (one, unless the plan's forms or input blob changed)
        self._warm = False      # an eager draw pass has run
        self.draws = None
        self.stream = torch.cuda.Stream(device=dev)  # capture needs a stream of its own

    def _score(self):
        """the plain likelihood of the pass just issued, folded into state"""
        p = self.plan
        p.losses(with_grad=False, combine=False, plain=True)
        o.iw_fold(p.eps, p.sigma, p.z, p.recon, self.recon_scale, self.state)

    def draw_pass(self):
        """one draw: the decoder half on a new eps, its likelihood, the fold (the kernel sequence of the captured graph)"""
        self.plan.forward(inference=True, start="latent")
        self._score()

    def graph_nodes(self):
        """(nodes, kernel launches among them) of the captured draw pass"""
        if self.graph is None:
            raise RuntimeError("no draw pass has been captured yet (run() with samples >= 3)")
        return self.graph.nodes, self.graph.kernel_nodes

    def _record(self, k):
        p, d = self.plan, self.draws
        for name in ("eps", "sigma", "z", "recon"):
            d[name][k].copy_(getattr(p, name))
        d["seed"][k].copy_(p.store.rng_state_inference()[0])

    def run(self, samples, keep_draws=False, reset_acc=False):
        """the bound of the batch in the plan's input buffers from `samples` draws; results() reads it. reset_acc: acc is cleared first
        (it then holds this batch's sums alone)"""
        check_iw(samples)
        p, K = self.plan, int(samples)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self.draws = None
            if keep_draws:
                f32 = dict(dtype=torch.float32, device=p.dev)
                Z = p.cfg.latent_dim
                self.draws = dict(eps=torch.zeros(K, p.B, Z, **f32), sigma=torch.zeros(K, p.B, Z, **f32), z=torch.zeros(K, p.B, Z, **f32),
                                  recon=torch.zeros(K, p.B, **f32), seed=torch.zeros(K, dtype=torch.int64, device=p.dev))
            o.zero(self.state)
            if reset_acc:
                o.zero(self.acc)
            p.forward(inference=True)  # encodes, and is draw 1
            self._score()
            if keep_draws:
                self._record(0)
            key = (p.forms, p.inbuf.data_ptr())
            for k in range(1, K):
                if keep_draws or not self._warm:
                    self.draw_pass()
                    self._warm = True
                    if keep_draws:
                        self._record(k)
                    continue
                if self.graph is None or self._graph_key != key:
                    self.graph, self._graph_key = o.Graph().capture(self.draw_pass), key
                    self.captures += 1
                self.graph.launch()
            o.iw_finish(self.state, self.out, self.acc)
        torch.cuda.current_stream().wait_stream(self.stream)  # the caller reads the results on its own stream
        return self

    def results(self):
        """per piece, as host arrays: log_px, elbo, ess, n (draws folded) and valid (False: a draw was not finite; the three figures are NaN)"""
        out = self.out.cpu().numpy()
        res = {name: out[:, i].copy() for i, name in enumerate(o.IW_OUT)}
        res["valid"] = ~np.isnan(out[:, 0])
        return res

    def read_acc(self, reset=True):
        """the six running sums (ops.IW_ACC) as a host array: one device->host read; iw_scores turns them into the reported figures"""
        acc = self.acc.cpu().numpy().copy()
        if reset:
            o.zero(self.acc)
        return acc
