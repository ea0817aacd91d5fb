"""Trainer with the reference's API (VarAutoEncoder/trainer.py:14-270): OptimizerConfig, TrainConfig,
TrainingState, Trainer(config, context, model, sampler).fit(dataset, model_folder, epochs, validation_dataset)
and ._step(batch, is_train).

_step is the hot path: ONE hipGraph replay runs forward, CE/BCE + kl_weight*KL, backward and the fused MXNet-rule Adam
(engine.StepPlan) on a batch that Trainer.fit's PinnedBatchPipeline packed into a page-locked ring slot and uploaded on a
side stream while the previous step ran; with several ranks the flat gradient bucket is all-reduced over RCCL in two
ranges, the first one under the rest of the backward pass. All five metrics of the reference (ppl, acc, topk, kl_loss,
total_loss) accumulate on the device and are read at log time only (the reference syncs three times per step,
trainer.py:181-186)."""
import contextlib
import os
from time import time

import numpy as np
import torch

from . import utils
from .config import Config
from .. import parallel
from ..step_math import (check_class_mmd, check_clip, check_ema, check_input_dropout, check_iw, check_schedule, class_mmd_score, iw_scores,
                         latent_scores, roll_scores)
from ..pianoroll import PinnedBatchPipeline


class OptimizerConfig(Config):
    def __init__(self, optimizer: str, optimizer_params: str, learning_rate: float):
        super().__init__()
        self.optimizer, self.optimizer_params, self.learning_rate = optimizer, optimizer_params, learning_rate

    def params_to_dict(self):
        """'k1:v1,k2:v2' -> {k1: float(v1), ...}; malformed pairs are skipped (trainer.py:23-35)"""
        out = {}
        for kv in self.optimizer_params.strip().split(","):
            kv = kv.split(":")
            if len(kv) == 2:
                out[str(kv[0])] = float(kv[1])
        return out


class TrainConfig(Config):
    """kl_warmup_steps / kl_cycle_steps / kl_free_bits / lr_warmup_steps: the training schedules (engine.schedule_values), all off at
    their defaults. clip_global_norm: bound on the global L2 norm of the gradient, applied inside the step (engine.clip_scale); 0: off.
    ema_decay: decay of the exponential moving average of the weights the step keeps (engine.ema_update), which validation, early
    stopping and the periodic samples then use; 0: off.
    d_input_dropout: probability that a training step hides a decoder input position from the teacher-forced decoder
    (engine.check_input_dropout; include/mst_hip.h: mst_step_begin_args.in_*), in [0, 1]; 0: off. Validation never drops.
    latent_stats: the steps keep per-class, per-dimension sums of the posterior's mu, sigma and KL on the device, and the metrics gain
    active_units, kl_dims_used, kl_dim_max, sigma_rms and class_leak (engine.latent_scores); False: off.
    iw_samples: K of the importance-weighted bound on log p(x) the trainer computes over the validation set after each checkpoint's
    validation pass (engine.IWBound, engine.iw_scores), an integer >= 1; 0: off. Early stopping still compares total_loss.
    class_mmd: multiplier lambda of the class-conditional MMD penalty on z the training steps add to their objective (include/mst_hip.h:
    mst_class_mmd); the metrics gain class_mmd, the mean penalty per batch, which early stopping does not look at. 0: off.
    class_mmd_bandwidth: the penalty kernel's bandwidth s2; 0: the latent width.
    YAML-serialisable (Config): a file written before a field existed loads with that field's default."""

    def __init__(self, batch_size: int, sampling_frequency: int, checkpoint_frequency: int, num_checkpoints_not_improved: int,
                 optimizer: OptimizerConfig, kl_loss: float, label_smoothing: float, negative_label_downscaling: bool,
                 verbose: bool, dtype: str = "bf16", max_steps: int = 0, kl_warmup_steps: int = 0, kl_cycle_steps: int = 0,
                 kl_free_bits: float = 0.0, lr_warmup_steps: int = 0, clip_global_norm: float = 0.0, ema_decay: float = 0.0,
                 d_input_dropout: float = 0.0, latent_stats: bool = False, iw_samples: int = 0, class_mmd: float = 0.0,
                 class_mmd_bandwidth: float = 0.0):
        super().__init__()
        if iw_samples != 0:
            check_iw(iw_samples)
        self.iw_samples = iw_samples
        check_schedule(kl_warmup_steps, kl_cycle_steps, kl_free_bits, lr_warmup_steps)
        check_clip(clip_global_norm)
        self.clip_global_norm = clip_global_norm
        check_ema(ema_decay)
        self.ema_decay = ema_decay
        check_input_dropout(d_input_dropout)
        self.d_input_dropout = d_input_dropout
        self.latent_stats = bool(latent_stats)
        check_class_mmd(class_mmd, class_mmd_bandwidth)
        self.class_mmd, self.class_mmd_bandwidth = float(class_mmd), float(class_mmd_bandwidth)
        self.kl_warmup_steps, self.kl_cycle_steps = kl_warmup_steps, kl_cycle_steps
        self.kl_free_bits, self.lr_warmup_steps = kl_free_bits, lr_warmup_steps
        self.batch_size = batch_size
        self.sampling_frequency = sampling_frequency
        self.checkpoint_frequency = checkpoint_frequency
        self.num_checkpoints_not_improved = num_checkpoints_not_improved
        self.optimizer = optimizer
        self.kl_loss_weight = kl_loss
        self.label_smoothing = label_smoothing
        self.negative_label_downscaling = negative_label_downscaling
        self.verbose = verbose
        self.dtype = dtype
        self.max_steps = max_steps


class TrainingState:
    def __init__(self):
        self.n_checkpoints = 0
        self.n_batches = 0
        self.num_checkpoints_not_improved = 0
        self.best_resconstruction_loss = np.inf


class Trainer:
    def __init__(self, config: TrainConfig, context, model, sampler=None):
        self.config, self.context, self.model, self.sampler = config, context, model, sampler
        if config.optimizer.optimizer != "adam":
            raise ValueError("only the 'adam' optimizer of scripts/train-vae.sh is implemented")
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        device = getattr(context, "device", context)
        if torch.device(device).type != "cuda":
            raise RuntimeError("the VarAutoEncoder step runs on hand-written HIP kernels only: no CPU path exists "
                               "(pass --gpu / a HIP device)")
        # THIS rank's GPU becomes the current device before anything touches HIP: the process group binds to it, and
        # every launch goes to torch's current stream of the current device (ops.ptr refuses tensors of another card)
        torch.cuda.set_device(device)
        utils.limit_host_threads()
        self.dist = parallel.init_process_group(self.world, self.rank) if self.world > 1 else None
        self.reduce_fn = parallel.make_grad_allreduce(self.dist) if self.dist is not None else None
        # data parallel: asynchronous two-range all-reduce overlapped with the tail of backward (engine.StepPlan.capture)
        self.reducer = parallel.GradReducer(self.dist) if self.dist is not None else None
        # the step runs (and is captured) on its own stream: the legacy default stream cannot be captured. Everything that
        # touches the model's device state — parameter upload, checkpoint load, metric reads, the sampler — runs under it
        # too, so one stream orders all of it.
        self.stream = torch.cuda.Stream(device=device)
        with torch.cuda.stream(self.stream):
            self._initialize_model()
        self._initialize_optimizers()
        if self.ema_decay > 0:
            with torch.cuda.stream(self.stream):
                self.model.store.enable_ema()  # (a copy of the initial weights; a checkpoint found by fit() replaces it)
        self.stream.synchronize()
        self._graphs = {}
        self._tail_gen = 0
        self.model.on_plan_evicted(self._forget_plan)
        # a failed one-launch position-0 tail (engine.ParamStore.handle_step_status) switches the store to the five-launch form:
        # the graphs recorded with the old kernel sequence are dropped and every shape runs one eager step again (lazy module
        # loads). With more than one rank a skipped update on one rank would let the replicas drift apart: stop instead.
        self.model.store.on_tail_failure(self._on_tail_failure)
        if self.world > 1:
            self.model.store.tail_policy = "raise"
        self.pipeline = PinnedBatchPipeline(self.model.store.device, lambda B, T: self._plan(B, T))
        self.train_state = TrainingState()
        self.summary_writer = utils.ScalarWriter(os.environ.get("MST_LOGDIR", "/tmp/out")) if self.rank == 0 else None
        self._grad_ranges = None

    def _initialize_model(self):
        """model.initialize(mx.init.Xavier(), ctx) (trainer.py:103-105); same seed on every rank"""
        adt = torch.bfloat16 if self.config.dtype == "bf16" else torch.float16
        self.model.initialize(self.context, act_dtype=adt)

    def _initialize_optimizers(self):
        """gluon.Trainer(params, 'adam', {learning_rate, **optimizer_params}) (trainer.py:94-101)"""
        extra = self.config.optimizer.params_to_dict()
        self.hyper = dict(lr=self.config.optimizer.learning_rate, clip_gradient=extra.get("clip_gradient", None),
                          kl_weight=self.config.kl_loss_weight, label_smoothing=self.config.label_smoothing,
                          negative_label_downscaling=self.config.negative_label_downscaling, internal_eps=True)
        # the training schedules join the plan's hyper-parameters (and with them the plan cache's key) only when one is on
        sched = {k: getattr(self.config, k, 0) for k in ("kl_warmup_steps", "kl_cycle_steps", "kl_free_bits", "lr_warmup_steps")}
        check_schedule(**sched)
        self.scheduled = any(sched.values())
        if self.scheduled:
            self.hyper.update(sched)
        # ... and so does clipping by the global gradient norm
        self.clip_global_norm = float(getattr(self.config, "clip_global_norm", 0.0))
        check_clip(self.clip_global_norm)
        if self.clip_global_norm > 0:
            self.hyper["clip_global_norm"] = self.clip_global_norm
        # ... and the exponential moving average of the weights
        self.ema_decay = float(getattr(self.config, "ema_decay", 0.0))
        check_ema(self.ema_decay)
        if self.ema_decay > 0:
            self.hyper["ema_decay"] = self.ema_decay
        # ... and decoder-input dropout
        self.d_input_dropout = float(getattr(self.config, "d_input_dropout", 0.0))
        check_input_dropout(self.d_input_dropout)
        if self.d_input_dropout > 0:
            self.hyper["d_input_dropout"] = self.d_input_dropout
            if self.rank == 0:
                print("Decoder-input dropout: a training step hides each decoder input position with probability {}".format(
                    self.d_input_dropout))
        # ... and the per-dimension latent statistics (not a hyper-parameter: a flag of the plan, set in _plan)
        self.latent_stats = bool(getattr(self.config, "latent_stats", False))
        self.last_latent_stats = None  # engine.latent_scores of the latest collect_metrics()
        # ... and the class-conditional MMD penalty on z (two fields of the plan, set in _plan: no new buffer, no other launch form)
        self.class_mmd = float(getattr(self.config, "class_mmd", 0.0))
        self.class_mmd_bandwidth = float(getattr(self.config, "class_mmd_bandwidth", 0.0))
        check_class_mmd(self.class_mmd, self.class_mmd_bandwidth)
        if self.class_mmd > 0 and self.rank == 0:
            print("Class MMD penalty on z: lambda {}, bandwidth {}".format(self.class_mmd, self.class_mmd_bandwidth or "Z"))
        # ... and the importance-weighted bound over the validation set (not a hyper-parameter either: _iw_validation)
        self.iw_samples = getattr(self.config, "iw_samples", 0)
        if self.iw_samples != 0:
            check_iw(self.iw_samples)
        self._iw_acc = None  # the six fp64 sums every IWBound of a validation adds to, made at first use
        self.opt_extra = {k: v for k, v in extra.items() if k in ("beta1", "beta2", "epsilon", "wd")}

    # ------------------------------------------------------------------ the hot loop
    def _plan(self, B, T):
        """the StepPlan of a per-rank batch shape. Every rank uses the SAME step seed; eps is drawn per global sample index
        (sample_offset) so the result does not depend on the sharding, and the dropout site ids are offset per rank so the
        ranks' masks differ."""
        plan = self.model.plan(B, T, global_batch=B * self.world, seed=1000, sample_offset=self.rank * B,
                               site_base=64 * self.rank, **self.hyper)
        if not getattr(plan, "_trainer_set", False):
            for src, dst in (("beta1", "beta1"), ("beta2", "beta2"), ("epsilon", "eps"), ("wd", "wd")):
                if src in self.opt_extra:
                    plan.opt[dst] = self.opt_extra[src]
            plan.track_token_metrics = plan.cfg.kind == "token"  # ppl / acc / topk sums ride on the CE launch
            plan.track_roll_metrics = plan.cfg.kind == "pianoroll"  # tp / pred / pos / cells counts ride on the BCE launch
            plan.track_latent_stats = self.latent_stats  # per-dimension sums of mu / sigma / KL: one launch behind the latent block's
            plan.class_mmd, plan.class_mmd_s2 = self.class_mmd, self.class_mmd_bandwidth or None  # lambda * L joins the training objective
            plan._trainer_set = True
        return plan

    GUARD_POLL_STEPS = 4  # steps between two non-blocking looks at the step guard's status words

    def _poll_guard(self):
        """ParamStore.poll_status every few steps: a failed one-launch tail switches the run to the five-launch form within
        2 x GUARD_POLL_STEPS steps instead of at the next periodic log (each step in between is a skipped batch). Data
        parallel: the words are summed over the ranks first (one 8-byte all-reduce per poll), and every rank stops."""
        with torch.cuda.stream(self.stream):
            self.model.store.poll_status(reduce=(lambda t: self.dist.all_reduce(t)) if self.dist is not None else None)

    def _on_tail_failure(self):
        self._graphs.clear()
        self._tail_gen += 1

    def _forget_plan(self, plan):
        for k in [k for k in self._graphs if k[0] == id(plan)]:
            del self._graphs[k]
        self.pipeline.drop(plan)

    def _averaged(self):
        """the context validation and the periodic sampler run in: the averaged weights swapped in (ParamStore.ema_weights, on the
        trainer's stream), or nothing at all without ema_decay"""
        return self.model.store.ema_weights() if self.ema_decay > 0 else contextlib.nullcontext()

    def _shard(self, batch):
        return parallel.shard_bounds(len(batch.data[1]), self.world, self.rank) if self.world > 1 else None

    def _run(self, plan, inbuf, is_train):
        """one step of `plan` reading the device blob `inbuf`: the first step of a shape runs eagerly (HIP modules load
        lazily and are not capturable), every (plan, input blob, mode) gets its own captured graph(s), later steps replay"""
        if plan.inbuf.data_ptr() != inbuf.data_ptr():
            plan.bind_inputs(inbuf)
        key = (id(plan), inbuf.data_ptr(), is_train)
        g = self._graphs.get(key)
        ran = False
        warm = plan.__dict__.setdefault("_warm", set())
        if (is_train, self._tail_gen) not in warm:
            plan.step_kernels(is_train, reduce_fn=self.reduce_fn)
            self.stream.synchronize()
            warm.add((is_train, self._tail_gen))
            ran = True
        if g is None:
            plan.capture(is_train, split_optimizer=self.world > 1, overlap=self.world > 1)
            g = self._graphs[key] = (plan.graph, plan.graph_late, plan.graph_opt)
        if not ran:
            plan.graph, plan.graph_late, plan.graph_opt = g
            plan.run(reduce_fn=self.reduce_fn if is_train else None, reducer=self.reducer if is_train else None)

    def _step(self, batch, is_train=True, staged=None):
        """trainer.py:155-179. `staged`: the batch as PinnedBatchPipeline uploaded it (Trainer.fit); without it the batch
        is copied into the plan's own input buffers here (validation, direct callers)."""
        with torch.cuda.stream(self.stream):
            if staged is not None:
                plan, slot = staged.plan, staged.slot
                self.stream.wait_event(slot.uploaded)
                self._run(plan, slot.dev, is_train)
                slot.consumed.record(self.stream)
            else:
                tokens, seq_lens, classes = batch.data
                labels = batch.label[0]
                shard = self._shard(batch)
                if shard is not None:  # contiguous shard of the global batch; padded length stays global (loss.py:23)
                    lo, hi = shard
                    tokens, seq_lens, classes, labels = tokens[lo:hi], seq_lens[lo:hi], classes[lo:hi], labels[lo:hi]
                plan = self._plan(tokens.shape[0], tokens.shape[1])
                plan.bind_inputs(plan.own_inbuf)
                plan.load_batch(tokens, seq_lens, classes, labels)
                self._run(plan, plan.own_inbuf, is_train)
        if self.config.verbose:
            print("Step {}: batch {} x {}".format(self.train_state.n_batches, plan.B, plan.T))
        self._last_plan = plan

    def fit(self, dataset, model_folder: str, epochs: int, validation_dataset=None):
        start_time = time()
        self.train_state = TrainingState()
        self._load_latest_checkpoint(model_folder)
        self._last_dataset = dataset
        for epoch in range(epochs):
            # the batcher runs one batch ahead: batch i+1 is packed into a page-locked ring slot and uploaded on the
            # pipeline's stream while the captured graph of step i executes (data.py:181-198 -> trainer.py:156-157)
            for staged in self.pipeline.feed(dataset, self._shard if self.world > 1 else None):
                batch = staged.batch
                self._step(batch, staged=staged)
                self.train_state.n_batches += 1
                if self.train_state.n_batches % self.GUARD_POLL_STEPS == 0:
                    self._poll_guard()
                if self.train_state.n_batches % 50 == 0:
                    self._periodic_log(epoch, start_time)
                if self.config.checkpoint_frequency > 0 and self.train_state.n_batches % self.config.checkpoint_frequency == 0:
                    self._checkpoint(model_folder, validation_dataset)
                    if self.train_state.num_checkpoints_not_improved == self.config.num_checkpoints_not_improved:
                        print("Maximum checkpoints not improved reached. Stopping training.")
                        return
                if (self.sampler is not None and self.config.sampling_frequency > 0
                        and self.train_state.n_batches % self.config.sampling_frequency == 0):
                    with torch.cuda.stream(self.stream), self._averaged():  # ordered behind the step that just updated the weights
                        self.sampler.update_parameters(self.model)
                        self.sampler.process_batch(batch, os.path.join(model_folder, "samples/step-{}".format(self.train_state.n_batches)),
                                                   dataset.num_classes())
                if self.config.max_steps and self.train_state.n_batches >= self.config.max_steps:
                    return

    # ------------------------------------------------------------------ metrics / logging
    def collect_metrics(self, reset=True):
        """the reference's five metrics over every step since the last reset (trainer.py:107-120,181-186): kl_loss /
        total_loss batch means and, for the token ends, masked ppl / acc / topk, for the piano-roll ends precision / recall / f1 / cell_acc
        of the predicted notes (engine.roll_scores of the counts the loss launches keep; early stopping still compares total_loss) — all accumulated on the device by the
        steps themselves and read here with one synchronisation. kl_weight / lr_scale: the KL weight and the learning-rate factor
        of the last training step, from the device schedule block in the same read (the configured constants without schedules;
        computed per rank from the same step count, so there is nothing to reduce). With clip_global_norm on, also grad_norm (the mean
        gradient norm before clipping over those steps), grad_norm_max and clip_frac: taken from the all-reduced bucket, the same on
        every rank, so nothing to reduce either. With latent_stats on, also active_units, kl_dims_used, kl_dim_max, sigma_rms and
        class_leak (engine.latent_scores of the per-class, per-dimension sums the steps keep, summed over the ranks with the rest);
        the whole dict of that read, the per-dimension KL included, stays in last_latent_stats. With class_mmd on, also class_mmd (the
        mean penalty L per counted batch; data parallel: over every rank's shards, each penalised on its own) and class_mmd_bad (batches
        whose L was not finite): engine.class_mmd_score of three more sums in the same all-reduce. total_loss stays recon + beta * kl."""
        failure = None
        with torch.cuda.stream(self.stream):  # ordered behind every step launched so far
            try:
                m = self.model.store.read_metrics(reset)
            except RuntimeError as e:  # (tail_policy "raise": data parallel) — tell the other ranks before stopping
                if self.dist is None:
                    raise
                failure = e
                m = self.model.store.read_metrics(reset)
        kl_weight, lr_scale = ((m.get("kl_weight", self.config.kl_loss_weight), m.get("lr_scale", 1.0)) if self.scheduled
                               else (self.config.kl_loss_weight, 1.0))
        gnorm = {k: m[k] for k in ("grad_norm", "grad_norm_max", "clip_frac") if k in m} if self.clip_global_norm > 0 else {}
        keys = [k for k in ("kl_sum", "total_sum", "count", "nll_sum", "acc_hits", "topk_hits", "n_tokens", "roll_tp", "roll_pred", "roll_pos",
                            "roll_cells") if k in m]  # (the counts: float64 is exact far beyond any run's)
        lat = m["lat_stats"] if self.latent_stats else None  # fp64 [classes, 5, Z] sums: they add over the ranks like the rest
        mmd = np.asarray(m["class_mmd_acc"], np.float64) if self.class_mmd > 0 else None  # {sum L, batches, bad batches}
        if self.dist is not None:
            with torch.cuda.stream(self.stream):
                t = torch.tensor([m[k] for k in keys] + [1.0 if failure is not None else 0.0] + (mmd.tolist() if mmd is not None else [])
                                 + (lat.ravel().tolist() if lat is not None else []), dtype=torch.float64, device=self.model.store.device)
                self.dist.all_reduce(t)
                vals = t.tolist()
                m = dict(zip(keys, vals))
                failed = vals[len(keys)]
                at = len(keys) + 1
                if mmd is not None:
                    mmd, at = np.asarray(vals[at: at + 3], np.float64), at + 3
                if lat is not None:
                    lat = np.asarray(vals[at:], np.float64).reshape(lat.shape)
            if failed > 0:
                raise RuntimeError(f"{int(failed)} rank(s) skipped optimizer steps after a failed position-0 tail; the replicas "
                                   "are no longer identical — restart from the last checkpoint with MST_ROW_TAIL=0"
                                   + (f" (this rank: {failure})" if failure is not None else ""))
        out = {}
        if "n_tokens" in m:
            n = m["n_tokens"]
            out["ppl"] = float(np.exp(m["nll_sum"] / n)) if n else float("nan")
            out["acc"] = m["acc_hits"] / n if n else float("nan")
            out["topk"] = m["topk_hits"] / n if n else float("nan")
        if "roll_cells" in m:  # piano-roll ends: precision / recall / f1 / cell_acc of the notes the decoder predicts (logit > 0)
            out.update(roll_scores(*(int(m[k]) for k in ("roll_tp", "roll_pred", "roll_pos", "roll_cells"))))
        n = max(m["count"], 1.0)
        out["kl_loss"] = m["kl_sum"] / n
        out["total_loss"] = m["total_sum"] / n
        out["kl_weight"], out["lr_scale"] = kl_weight, lr_scale
        out.update(gnorm)
        if lat is not None:
            self.last_latent_stats = latent_scores(lat)
            out.update({k: self.last_latent_stats[k] for k in ("active_units", "kl_dims_used", "kl_dim_max", "sigma_rms", "class_leak")})
        if mmd is not None:
            out.update(class_mmd_score(mmd))
        return out

    def _metric_to_string_output(self, n_batches):
        """trainer.py:239-248: every metric goes to the scalar log and into the printed line, then is reset"""
        out = ""
        for name, val in self.collect_metrics(reset=True).items():
            if self.summary_writer is not None:
                self.summary_writer.add_scalar(tag=name, value=val, global_step=n_batches)
            out += "{}={:.3f} ".format(name, val)
        return out

    def _periodic_log(self, epoch, start_time):
        line = self._metric_to_string_output(self.train_state.n_batches)
        if self.rank == 0:
            print("Epoch [{}] Batch [{}] updates/sec: {:.2f} {}".format(
                epoch, self.train_state.n_batches, self.train_state.n_batches / (time() - start_time), line), flush=True)
        self._log_gradients()
        if self.summary_writer is not None:
            self.summary_writer.flush()

    def gradient_norms(self):
        """name -> L2 norm of the parameter's gradient as the last step left it (sum over the global batch, before the
        1/B rescale: what grad.grad().norm() is in trainer.py:257-265) — ONE launch over the flat bucket + one read"""
        st = self.model.store
        plan = self._last_plan
        with torch.cuda.stream(self.stream):
            if self._grad_ranges is None:
                r = [[st.offsets[n], st.offsets[n] + int(np.prod(s))] for n, s in st.shapes.items()]
                self._grad_ranges = torch.tensor(r, dtype=torch.int64, device=st.device)
                self._grad_sumsq = torch.zeros(len(r), dtype=torch.float32, device=st.device)
            from .. import ops as o
            o.segment_sumsq(st.g, self._grad_ranges, self._grad_sumsq)
            ss = self._grad_sumsq.cpu().numpy()
        return {n: float(np.sqrt(v)) / (plan.gscale_enc if n.startswith("encoder.") else plan.gscale)
                for n, v in zip(st.shapes, ss)}

    def _log_gradients(self):
        """trainer.py:257-270: one scalar per parameter + their mean as 'global_grad'"""
        if self.summary_writer is None or getattr(self, "_last_plan", None) is None:
            return
        norms = self.gradient_norms()
        for name, v in norms.items():
            self.summary_writer.add_scalar(tag=name, value=v, global_step=self.train_state.n_batches)
        self.summary_writer.add_scalar(tag="global_grad", value=sum(norms.values()) / max(1, len(norms)),
                                       global_step=self.train_state.n_batches)

    def _iw_validation(self, validation_dataset):
        """The importance-weighted bound on log p(x) over the validation set from iw_samples draws per piece (engine.IWBound): called
        inside the validation's own context — the trainer's stream, the averaged weights where the run keeps them. Every batch's
        runner adds to the same six device sums, which are read once; data parallel: each rank scores its shard (eps per global sample
        index, plan.sample_offset) and the sums — with the cell and piece counts, in the same tensor — are all-reduced once, by every
        rank unconditionally. Inference passes on the store's inference RNG stream: the training steps after it are what they would
        have been. Returns engine.iw_scores' dict (cells per piece: the mean over the pieces scored); the figures also go to the scalar log."""
        st = self.model.store
        if self._iw_acc is None:
            self._iw_acc = torch.zeros(6, dtype=torch.float64, device=st.device)
        acc = self._iw_acc
        acc.zero_()
        cells = pieces = 0
        for batch in validation_dataset:
            tokens, seq_lens, classes = batch.data
            labels = batch.label[0]
            shard = self._shard(batch)
            if shard is not None:
                lo, hi = shard
                tokens, seq_lens, classes, labels = tokens[lo:hi], seq_lens[lo:hi], classes[lo:hi], labels[lo:hi]
            plan = self._plan(tokens.shape[0], tokens.shape[1])
            plan.bind_inputs(plan.own_inbuf)
            plan.load_batch(tokens, seq_lens, classes, labels)
            iw = self.model.iw_runner(plan, acc=acc).run(self.iw_samples)
            cells += plan.B * iw.cells
            pieces += plan.B
        t = torch.cat([acc, torch.tensor([cells, pieces], dtype=torch.float64, device=st.device)])
        if self.dist is not None:
            self.dist.all_reduce(t)
        sums = t.tolist()
        scores = iw_scores(sums[:6], sums[6] / sums[7] if sums[7] else 1.0)
        if self.summary_writer is not None:
            for name, val in scores.items():
                self.summary_writer.add_scalar(tag=name, value=val, global_step=self.train_state.n_batches)
        return scores

    # ------------------------------------------------------------------ checkpoint / resume (trainer.py:188-233)
    def _load_latest_checkpoint(self, model_folder):
        print("Looking into folder {} for a valid training.".format(model_folder))
        try:
            latest = utils.get_latest_checkpoint_index(model_folder)
        except (FileNotFoundError, OSError):
            print("No checkpoint was found. Starting training from scratch")
            return
        print("Checkpoint {} found. Resuming training.".format(latest))
        with torch.cuda.stream(self.stream):
            utils.load_model_parameters(self.model, os.path.join(model_folder, "params.{}".format(latest)), self.context)
            self.train_state = utils.load_object(os.path.join(model_folder, "train_state.pkl"))
            opt = os.path.join(model_folder, "optimizer.{}.npz".format(latest))
            averaged = False
            if os.path.exists(opt):  # Adam moments + step count (the reference does not save optimizer state)
                st = self.model.store
                with np.load(opt) as z:
                    st.m.copy_(torch.from_numpy(z["m"]))
                    st.v.copy_(torch.from_numpy(z["v"]))
                    st.step_state.copy_(torch.from_numpy(z["step_state"]))
                    if self.ema_decay > 0 and "ema" in z.files:
                        st.ema.copy_(torch.from_numpy(z["ema"]))
                        averaged = True
            if self.ema_decay > 0 and not averaged:  # (a run that did not average wrote it)
                self.model.store.load_ema_numpy(None)
                print("Checkpoint {} holds no averaged weights: the average starts from its parameters.".format(latest))
        self.stream.synchronize()

    def _checkpoint(self, model_folder, validation_dataset):
        self.train_state.n_checkpoints += 1
        n = self.train_state.n_checkpoints
        print("\nCheckpoint {} reached.".format(n))
        if self.rank == 0:
            with torch.cuda.stream(self.stream):  # reads ordered behind the last step
                utils.create_directory_if_not_present(model_folder)
                utils.save_model(self.model, os.path.join(model_folder, "params.{}".format(n)))
                utils.save_object(self.train_state, os.path.join(model_folder, "train_state.pkl"))
                st = self.model.store
                ema = dict(ema=st.ema.cpu().numpy()) if self.ema_decay > 0 else {}  # (params.N stays the raw weights)
                np.savez(os.path.join(model_folder, "optimizer.{}.npz".format(n)), m=st.m.cpu().numpy(), v=st.v.cpu().numpy(),
                         step_state=st.step_state.cpu().numpy(), **ema)
        self.collect_metrics(reset=True)
        if validation_dataset is None:
            return
        with torch.cuda.stream(self.stream), self._averaged():  # (with ema_decay: the averaged model is what early stopping compares)
            for batch in validation_dataset:
                self._step(batch, is_train=False)
            vals = self.collect_metrics(reset=True)
            if self.iw_samples > 0:
                vals.update(self._iw_validation(validation_dataset))
        loss = vals["total_loss"]
        if loss < self.train_state.best_resconstruction_loss:
            print("Loss improved from {} to {}.".format(self.train_state.best_resconstruction_loss, loss))
            self.train_state.best_resconstruction_loss = loss
        else:
            self.train_state.num_checkpoints_not_improved += 1
            print("Loss did not improve. {} out {} unsucessful checkpoints".format(
                self.train_state.num_checkpoints_not_improved, self.config.num_checkpoints_not_improved))
            print("Best loss thus far: {}".format(self.train_state.best_resconstruction_loss))
        print("Checkpoint [{}]  {}\n".format(n, " ".join("{}={:.3f}".format(k, v) for k, v in vals.items())))
        self.last_validation = vals
