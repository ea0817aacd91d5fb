"""Incremental decoding with per-layer K | Q | V caches in HBM (reference model.py:107-128,259-272,
transformer.py:70-77,242-249, sampler.py:155-257).

The reference's own inference path is inconsistent with its decoder (`forward_inference` signatures do not
match the samplers, `compute_with_cache` never appends because the decoder's self-attention is built with
mask_future_timesteps=False, `mx.nd.concat([..], axis=1)` is a wrong call), so this is the evident intent, restated once in
oracle/vae_oracle.py::decode_incremental and implemented here on the same kernels as the training step:

  * position 0 is the initial state row, sqrt(D) * (latent2hid(z) + class2hid(c)) + pos[0] (model.py:229-232,
    transformer.py:237) — exactly what mst_latent_fwd writes as decoder row 0 in training;
  * position t >= 1 embeds the previous token (or frame) with pos[t] (transformer.py:246) and runs the layers on that ONE row
    per sample; each layer's K | Q | V projection of the row is written straight into its cache at row t by the projection
    GEMM's output row remap (no concat, no copy), and the new query attends to rows 0..t (mst_attn_decode);
  * attention arithmetic is the reference's: the softmax runs over the QUERY axis (transformer.py:100), which in a decode
    step holds the single new query — every weight is 1 and the head output is the sum of the cached value rows
    (mode 'query'); the conventional softmax over the cached keys is offered as mode 'key';
  * dropout layers are identities outside autograd.record() (inference).
Everything is one row per sample: the GEMMs are launch-bound M = B problems of the same mst_gemm_nt used in training, so a
position is ~8 launches per layer of a few microseconds each. Every position is therefore captured ONCE as a hipGraph (its
kernel arguments — the cache row written, the number of keys attended to, the positional row — are host scalars that differ
per position, hence one graph per position, captured by PositionGraphs.run — the one place) and replayed from then on; plans are
kept per (hypotheses, positions, attention mode) by the model, so beam search over many batches captures nothing twice."""
import contextlib
import math
import os

import numpy as np
import torch

from . import ops as o
from .MIDIUtil.defaults import EOS_ID, PAD_ID, SOS_ID
from .layer_block import ALL_ROWS, NO_DROPOUT, row_block_fwd
from .ops import roundup
from .spec import positional_table


class PositionGraphs:
    """A position's kernel sequence, eager once, then a captured graph: the key -> ops.Graph dict and the warm state of ONE owner
    (DecodePlan, BeamSearch, FrameSampling and TokenSampling each hold their own). A key is captured once its lane is warm, i.e. once a
    sequence of that lane has run eagerly here: HIP modules load lazily and cannot be loaded inside a capture. capture_behind: the
    eager position is captured right behind its eager run (not launched), so the next run replays it too; otherwise it is captured
    when a later run reaches it. `plan.use_graphs` is read at every position (off: eager launches, no key ever)."""

    def __init__(self, plan, capture_behind=False):
        self.plan, self.capture_behind = plan, capture_behind
        self.graphs, self.warm = {}, set()

    def run(self, key, fn, lane=False, warms=True):
        """warms=False: this eager run does not touch every kernel of the lane's later keys"""
        use = self.plan.use_graphs
        g = self.graphs.get(key) if use else None
        if g is None:
            if not (use and lane in self.warm):
                fn()
                if warms:
                    self.warm.add(lane)
                if use and self.capture_behind:
                    self.graphs[key] = o.Graph().capture(fn)
                return
            g = self.graphs[key] = o.Graph().capture(fn)
        g.launch()  # (all a captured position costs the host: one lookup, one launch)


class DecodePlan:
    """Buffers and the kernel sequence of incremental decoding for B hypotheses and up to t_max positions."""

    MODES = {"query": 0, "key": 1}

    def __init__(self, store, B, t_max, attention="query", pingpong=False):
        """pingpong: two sets of caches, position t working on set t & 1 — beam search on the device re-ranks the hypotheses
        after every position by gathering the cache rows from one set into the other (BeamSearch below)"""
        cfg = store.cfg
        self.store, self.cfg, self.B, self.t_max = store, cfg, B, t_max
        self.pingpong = pingpong
        self.mode = self.MODES[attention]
        dev, adt = store.device, store.act_dtype
        D = cfg.d_model
        self.pos = torch.from_numpy(positional_table(D, t_max)).to(dev)

        def act(rows, width):
            return torch.zeros(rows, roundup(width, 8), dtype=adt, device=dev)

        self.cache_sets = [[torch.zeros(B, t_max, 3 * D, dtype=adt, device=dev) for _ in range(cfg.d_layers)] for _ in range(2 if pingpong else 1)]
        self.cache = self.cache_sets[0]
        self.x, self.att, self.h1, self.x1, self.h2, self.x2 = (act(B, D) for _ in range(6))
        self.a = act(B, 4 * D)
        # W_proj + LN1 + feed-forward + LN3 of a position as ONE launch (the training step's mst_proj_ffn_ln_fwd) instead of
        # five: a decoded position is launch-floor bound (MST_DECODE_FFN=0: the five launches)
        self.fuse_ffn = o.can_fuse_ffn(D, 4 * D) and os.environ.get("MST_DECODE_FFN", "1") != "0"
        stat = lambda: torch.zeros(B, dtype=torch.float32, device=dev)
        self.mean2, self.rstd2 = stat(), stat()
        # (LayerNorm statistics, which nothing in decoding reads: a pair per LayerNorm for the one launch, which writes both; the five
        # launches write one pair after the other)
        self.mean1, self.rstd1 = (stat(), stat()) if self.fuse_ffn else (self.mean2, self.rstd2)
        self.logits = act(B, cfg.out_dim)
        self.loss = torch.zeros(B, dtype=torch.float32, device=dev)
        self.npos = torch.zeros(B, dtype=torch.int32, device=dev)
        if cfg.kind == "token":
            self.probs = torch.zeros(B, cfg.out_dim, dtype=torch.float32, device=dev)
            self.tokens = torch.zeros(B, 1, dtype=torch.int32, device=dev)
            self.zero_labels = torch.zeros(B, dtype=torch.int32, device=dev)
        else:
            self.probs = act(B, cfg.out_dim)
            self.frames = torch.zeros(B, roundup(cfg.in_dim, 8), dtype=torch.uint8, device=dev)
            self.zero_labels = torch.zeros(B, cfg.out_dim, dtype=torch.uint8, device=dev)
        self.t = -1  # position of the last row fed
        # one captured graph per position (MST_DECODE_GRAPHS=0: eager launches); capture needs a stream of its own
        self.use_graphs = os.environ.get("MST_DECODE_GRAPHS", "1") != "0"
        self.stream = torch.cuda.Stream(device=dev)
        self._runner = PositionGraphs(self)
        self._graphs = self._runner.graphs  # position -> ops.Graph

    # ------------------------------------------------------------------ one position through the decoder layers
    def _layers(self, x, t):
        cfg, st, B = self.cfg, self.store, self.B
        D, H = cfg.d_model, cfg.d_heads
        for i in range(cfg.d_layers):
            P = st.layer("decoder", i)
            cache = self.cache_sets[(t & 1) if self.pingpong else 0][i]
            # K | Q | V of the new row, written to row t of every sample's cache (C row remap: logical row b -> b * t_max + t)
            o.gemm_nt(x, P.kqv.w, cache.view(B * self.t_max, 3 * D), M=B, K=D, bias=P.kqv.b, c_remap=(1, self.t_max, t))
            o.attn_decode(cache, t + 1, H, D // H, 0, D, 2 * D, self.att, mode=self.mode)
            # the training step's row-wise block on this plan's one-row buffers (att, h1, x1, a, h2, x2, mean1/2, rstd1/2);
            # transformer.py:199-200: LN3(ff + dropout(ff)) — dropout is the identity here, so 2 * ff
            row_block_fwd(P, self, x, ALL_ROWS, NO_DROPOUT, "fused" if self.fuse_ffn else "launches")
            x = self.x2 if i == cfg.d_layers - 1 else self._keep(self.x2)
        return x

    def _keep(self, x2):
        """the next layer's input must survive that layer's own writes to x2"""
        self.x.copy_(x2)
        return self.x

    # ------------------------------------------------------------------ API
    def _enter(self):
        self.stream.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self.stream)

    def _leave(self):
        torch.cuda.current_stream().wait_stream(self.stream)  # the caller reads the results on its own stream

    def reset(self):
        """forget the positions fed so far (the caches are overwritten from row 0 on); captured graphs stay valid"""
        self.t = -1

    def start(self, row0):
        """position 0: the initial state rows [B, >= D] (16-bit), ALREADY scaled and positioned as the training step's
        decoder row 0 (engine.StepPlan.x0_d[:, 0]); fills row 0 of every layer's cache"""
        with self._enter():
            self.x.copy_(row0[:, : self.x.shape[1]])
            self._run_position(0)
        self._leave()
        self.t = 0

    def _position(self, t, probs=True):
        """the kernel sequence of position t >= 0 on inputs already in self.x (t = 0) / self.tokens / self.frames
        (probs=False: stop at the logits — FrameSampling's draw reads those)"""
        cfg, st, B = self.cfg, self.store, self.B
        D = cfg.d_model
        if t == 0:
            self._layers(self.x, 0)
            return
        sq = math.sqrt(float(D))
        if cfg.kind == "token":
            o.embed_fwd(self.tokens, st.p("decoder.embedding.weight"), self.pos[t:], self.x.view(B, 1, -1), 0, sq)
        else:
            o.gemm_nt(self.frames, st.t("decoder.embedding.weight"), self.x, N=D, alpha=sq, rowadd=self.pos[t:], rowadd_period=1)
        x = self._layers(self.x, t)
        o.gemm_nt(x, st.h("decoder.output_layer.weight"), self.logits, K=D, bias=st.p("decoder.output_layer.bias"))
        if not probs:
            return
        if cfg.kind == "token":
            # (pre_zeroed: only the probabilities are used here — no 4.7 us memset of a loss nobody reads in every position)
            o.softmax_ce(self.logits, self.zero_labels, self.loss, B, 1, cfg.out_dim, probs=self.probs, pre_zeroed=True)
        else:
            o.sigmoid_bce(self.logits, self.zero_labels, self.loss, B, 1, cfg.out_dim, npos=self.npos, probs=self.probs, pre_zeroed=True)

    def _run_position(self, t):
        """replay position t's graph (captured at first use once the plan has run a position >= 1 eagerly: position 1 has
        touched every kernel of a later position, position 0 has not)"""
        self._runner.run(t, lambda: self._position(t), warms=t >= 1)

    def step(self, prev):
        """position t = previous + 1: `prev` is the token fed at this position ([B] ids, token ends) or the frame ([B, P]
        {0,1}); returns the output distribution of this position, [B, V] fp32 probabilities (token ends) or [B, P] 16-bit
        per-pitch probabilities (piano-roll ends)"""
        cfg, B = self.cfg, self.B
        t = self.t + 1
        if t >= self.t_max:
            raise RuntimeError(f"decode buffers hold {self.t_max} positions")
        host = torch.as_tensor(np.asarray(prev.cpu() if torch.is_tensor(prev) else prev))
        with self._enter():
            if cfg.kind == "token":
                self.tokens.copy_(host.to(torch.int32).view(B, 1))
            else:
                self.frames[:, : cfg.in_dim].copy_(host.to(torch.uint8))
            self._run_position(t)
        self._leave()
        self.t = t
        return self.probs[:, : cfg.out_dim]

    def reorder(self, index):
        """beam search driven from the host: hypothesis j continues hypothesis index[j] — gather the caches' rows
        (sampler.py:236-238)"""
        assert not self.pingpong
        idx = torch.as_tensor(np.asarray(index), dtype=torch.int64, device=self.store.device)
        n = self.t + 1
        with self._enter():
            for i, c in enumerate(self.cache):
                c[:, :n] = c[:, :n].index_select(0, idx)
        self._leave()


class _Sampler:
    """What the runs of the device samplers below share. Every sampler has a DecodePlan of its own (`plan`) of which only position 0
    goes through _run_position: that plan never warms, so position 0 stays eager. The positions >= 1 go through the sampler's own
    PositionGraphs (AncestralSampling: eager launches)."""

    eos, pad, sos = EOS_ID, PAD_ID, SOS_ID

    def _seed_words(self, dev):
        """the draw's seed as a device word, which the host rewrites before a run through its pinned twin"""
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=dev)
        self._seed_host = torch.zeros(1, dtype=torch.int64).pin_memory()

    def _run_length(self, length):
        length = self.L if length is None else int(length)
        if not 2 <= length <= self.L:
            raise ValueError(f"length {length} outside [2, {self.L}]")
        return length

    @contextlib.contextmanager
    def _started(self, row0, seed=None):
        """the frame of a run, as `with self._started(row0) as p:` — on the plan's stream: the seed word rewritten (samplers that have
        one), row0 fed, position 0 run; the body issues the later positions and copies its results back, then the caller's stream
        waits for the plan's"""
        p = self.plan
        p.reset()
        with p._enter():
            if seed is not None:
                seed &= 0xFFFFFFFFFFFFFFFF
                self._seed_host[0] = seed - (1 << 64) if seed >= (1 << 63) else seed  # (an int64 word: two's complement)
                self.seed_word.copy_(self._seed_host, non_blocking=True)
            p.x.copy_(row0[:, : p.x.shape[1]])
            p._run_position(0)
            p.t = 0
            yield p
        p._leave()

    def _sos_rows(self, seqs, scores, first=None):
        """the token samplers' rows before position 1: SOS, then PAD; the scores at `first` (None: zero)"""
        seqs.fill_(self.pad)
        seqs[:, 0] = self.sos
        if first is None:
            o.zero(scores)
        else:
            scores.copy_(first)

    def _load_held(self, given, hold):
        """the piece and the mask of a constrained run, as _constraint returned them, into the sampler's device buffers (allocated
        by the first such run), and held_dev zeroed. Called on the plan's stream."""
        if self.given is None:
            self.given, self.hold = self._held_buffers()
            self.held_dev = torch.zeros_like(self.scores)
        self._load_constraint(given, hold)
        o.zero(self.held_dev)

    def _read_held(self, held):
        if held:
            self.held_scores = self.held_dev.cpu().numpy()


class BeamSearch(_Sampler):
    """Beam search with everything of a position on the device (reference sampler.py:198-257): the decode step of the B x K
    hypotheses, their re-ranking (mst_beam_step: scores, token rows, the words fed next) and the gather of the layers' cache
    rows (mst_beam_gather) are ONE captured graph per position; the host launches graphs and looks at a device counter of
    running hypotheses every few positions. Token rows, scores and caches alternate between two buffers by position parity."""

    def __init__(self, store, B, K, i_max, attention="query"):
        self.B, self.K, self.i_max = B, K, i_max
        self.plan = DecodePlan(store, B * K, i_max + 1, attention=attention, pingpong=True)
        dev, N = store.device, B * K
        self.seqs = [torch.zeros(N, i_max, dtype=torch.int32, device=dev) for _ in range(2)]
        self.scores = [torch.zeros(N, dtype=torch.float32, device=dev) for _ in range(2)]
        self.hyp = torch.zeros(N, dtype=torch.int32, device=dev)
        self.ident = torch.arange(N, dtype=torch.int32, device=dev)
        self.active = torch.zeros(i_max + 1, dtype=torch.int32, device=dev)
        first = torch.full((B, K), float("inf"))
        first[:, 0] = 0.0  # the K copies of a sample start identical: only the first one may expand
        self.first_scores = first.reshape(-1).to(dev)
        self._runner = PositionGraphs(self.plan)
        self._graphs = self._runner.graphs  # position -> ops.Graph
        self.positions = 0

    def _position(self, i):
        p = self.plan
        cur, nxt = i & 1, (i + 1) & 1
        p._position(i)
        o.beam_step(p.probs, self.scores[cur], self.scores[nxt], self.seqs[cur], self.seqs[nxt], self.hyp, p.tokens, i, self.K, self.eos,
                    self.pad, active=self.active)
        D = p.cfg.d_model
        for cin, cout in zip(p.cache_sets[cur], p.cache_sets[nxt]):
            o.beam_gather(cin, cout, self.hyp, i + 1, skip_cols=(D, D))  # K and V only: a past position's Q is never read again

    def run(self, row0, check_every=8):
        """row0: [B * K, >= D] initial decoder rows (every sample's row repeated K times). Returns (token rows [B*K, n] int32,
        scores [B*K] fp32) as host arrays, hypotheses of a sample best first."""
        with self._started(row0) as p:              # position 0 fills cache set 0, row 0 ...
            for cin, cout in zip(p.cache_sets[0], p.cache_sets[1]):
                o.beam_gather(cin, cout, self.ident, 1)  # ... which position 1 expects in set 1
            self._sos_rows(self.seqs[1], self.scores[1], self.first_scores)
            p.tokens.fill_(self.sos)
            o.zero(self.active)
            last = 0
            for i in range(1, self.i_max):
                self._runner.run(i, lambda: self._position(i))
                p.t = last = i
                if i % check_every == 0 and int(self.active[i].item()) == 0:
                    break                            # every hypothesis has ended (sampler.py: the loop's exit test)
            res = (last + 1) & 1
            got = self.seqs[res][:, : last + 1].cpu().numpy()
            scores = self.scores[res].cpu().numpy()
            live = self.active[: last + 1].cpu().numpy()
        # rows of width i_max like the host loop's (sampler.py:203): PAD behind the last decoded position
        seqs = np.full((got.shape[0], self.i_max), self.pad, got.dtype)
        seqs[:, : last + 1] = got
        self.positions = last
        # live continuations chosen per position (mst_beam_step's `active` counters): what was DECODED — a finished hypothesis's PAD
        # continuations and the up to check_every - 1 positions run after the last one ended are not tokens
        self.tokens_decoded = int(live[1:].sum())
        return seqs, scores


class AncestralSampling(_Sampler):
    """Ancestral sampling (sampler.py:155-190, token ends) with the draw on the device (mst_sample_step): the host neither
    sees the distributions nor feeds the tokens — it launches a position's kernels and polls a device counter of running
    sequences every few positions."""

    def __init__(self, store, B, i_max, attention="query", seed=0):
        self.B, self.i_max = B, i_max
        self.plan = DecodePlan(store, B, i_max + 1, attention=attention)
        dev = store.device
        self.seqs = torch.zeros(B, i_max, dtype=torch.int32, device=dev)
        self.scores = torch.zeros(B, dtype=torch.float32, device=dev)
        self.active = torch.zeros(i_max + 1, dtype=torch.int32, device=dev)
        self.seed, self.runs = int(seed), 0
        self.positions = 0

    def run(self, row0, check_every=8):
        """-> (token rows [B, n] int32, scores [B]) as host arrays. (Eager launches: the draw's seed changes from run to run and
        is a kernel argument; a position is the decode step's ~10 launches + one draw, with no host round trip in between.)"""
        self.runs += 1
        seed = (self.seed * 0x9E3779B97F4A7C15 + self.runs) & 0xFFFFFFFFFFFFFFFF
        with self._started(row0) as p:
            self._sos_rows(self.seqs, self.scores)
            o.zero(self.active)
            p.tokens.fill_(self.sos)
            last = 0
            for i in range(1, self.i_max):
                p._position(i)
                o.sample_step(p.probs, self.seqs, self.scores, p.tokens, i, seed, self.eos, self.pad, active=self.active)
                p.t = last = i
                if i % check_every == 0 and int(self.active[i].item()) == 0:
                    break
            seqs = self.seqs[:, : last + 1].cpu().numpy()
            scores = self.scores.cpu().numpy()
        self.positions = last
        return seqs, scores


class FrameSampling(_Sampler):
    """Sampling for the piano-roll ends with the whole position on the device (sampler.py:155-190 with a Bernoulli draw per pitch):
    the decode step of position i and mst_frame_step — which reads the position's logits, writes the frame where the next position's
    embedding GEMM reads it and into the roll, and adds the frame's -log p to the scores — are ONE captured graph per position. The
    draw's seed is a device word the host rewrites before a run, so the graphs captured by one run replay for every later one; the
    host sees nothing until the roll is copied back at the end. (The draw forms sigmoid(logit / tau) itself: these graphs have no
    sigmoid_bce launch.) tau, mode and thr are launch constants of mst_frame_step: a graph is kept per (position, tau, mode, thr).

    Constrained runs (run(..., given, hold)): cells of the piece are GIVEN — the position's graph ends in mst_frame_step_held, which
    writes a held cell from `given` instead of drawing it, so the decoder is fed the held cells as if it had drawn them and the caches
    and the arithmetic are the unconstrained path's. The mask and the piece are device buffers of the sampler (allocated at the first
    such run): the graph key gains one boolean and nothing else, another mask or piece captures nothing. The held cells' summed
    -log p is left in self.held_scores (host fp32 [N]) — it is not part of the returned scores."""

    def __init__(self, store, N, L, attention="query", keep_probs=False):
        """L positions: the start row + up to L - 1 frames. keep_probs: the per-position probabilities stay in self.probs
        (fp32 [N, L, P]; tests and diagnostics)"""
        cfg = store.cfg
        if cfg.kind == "token":
            raise ValueError("FrameSampling draws piano-roll frames; the token ends have AncestralSampling")
        if L < 2:
            raise ValueError("FrameSampling needs at least two positions")
        self.N, self.L, self.P = N, L, cfg.out_dim
        assert cfg.in_dim == cfg.out_dim, "a drawn frame is the next position's input"
        self.plan = DecodePlan(store, N, L, attention=attention)
        dev = store.device
        self.roll = torch.zeros(N, L, roundup(self.P, 8), dtype=torch.uint8, device=dev)
        self.scores = torch.zeros(N, dtype=torch.float32, device=dev)
        self.probs = torch.zeros(N, L, self.P, dtype=torch.float32, device=dev) if keep_probs else None
        self._seed_words(dev)
        self._runner = PositionGraphs(self.plan, capture_behind=True)
        self._graphs = self._runner.graphs  # (position, tau, mode, thr[, True: constrained]) -> ops.Graph
        self.given = self.hold = self.held_dev = None  # device buffers of constrained runs, allocated by the first one
        self.held_scores = None                        # host fp32 [N] of the latest constrained run

    def _position(self, i, tau, mode, thr, held=False):
        p = self.plan
        p._position(i, probs=False)
        if held:
            o.frame_step_held(p.logits, self.P, i, self.seed_word, p.frames, self.roll, self.scores, self.given, self.hold, self.held_dev,
                              tau=tau, mode=mode, thr=thr, probs_out=self.probs)
        else:
            o.frame_step(p.logits, self.P, i, self.seed_word, p.frames, self.roll, self.scores, tau=tau, mode=mode, thr=thr,
                         probs_out=self.probs)

    def _constraint(self, given, hold, length):
        """(given, hold) as host arrays [N, T, P], T <= length - 1 frames (row k is position k + 1's); frames behind T are free"""
        if given is None or hold is None:
            raise ValueError("a constrained run needs both `given` and `hold`")
        given, hold = np.asarray(given), np.asarray(hold)
        if given.shape != hold.shape or given.ndim != 3 or given.shape[0] != self.N or given.shape[2] != self.P:
            raise ValueError(f"given and hold must both be [{self.N}, frames, {self.P}], got {given.shape} and {hold.shape}")
        if given.shape[1] > length - 1:
            raise ValueError(f"{given.shape[1]} constrained frames for a run of {length - 1}")
        return given, hold

    def _held_buffers(self):
        self._given_host, self._hold_host = (torch.zeros(self.roll.shape, dtype=torch.uint8).pin_memory() for _ in range(2))
        return torch.zeros_like(self.roll), torch.zeros_like(self.roll)

    def _load_constraint(self, given, hold):
        """_load_held's copies: through pinned twins of the buffers' own layout, one contiguous transfer each. A cell is set where
        the byte is non-zero (the kernel's rule), so byte arrays go in as they are."""
        T = given.shape[1]
        for src, host, dev in ((given, self._given_host, self.given), (hold, self._hold_host, self.hold)):
            view = host.numpy()
            view[:, T:] = 0  # (frames behind T hold nothing; the pad columns stay zero)
            if src.dtype in (np.uint8, np.bool_):
                view[:, :T, : self.P] = src.view(np.uint8)
            else:
                np.not_equal(src, 0, out=view[:, :T, : self.P])
            dev.copy_(host, non_blocking=True)

    def run(self, row0, length=None, tau=1.0, mode="draw", thr=0.5, seed=0, given=None, hold=None):
        """row0: [N, >= D] initial decoder rows. Decodes positions 1 .. length - 1 (default: all L - 1) and returns
        (roll uint8 [N, length - 1, P], scores [N]) as host arrays: frame i - 1 is the draw of position i.
        given, hold: host arrays [N, T <= length - 1, P] in the returned roll's indexing: cell [n, k, j] of the roll is given[n, k, j]
        != 0 where hold[n, k, j] != 0 and drawn (or thresholded) elsewhere; the scores then sum the free cells only, and the held
        cells' cost is left in self.held_scores."""
        length = self._run_length(length)
        tau, thr = float(tau), float(thr)
        held = given is not None or hold is not None
        if held:
            given, hold = self._constraint(given, hold, length)
        with self._started(row0, seed) as p:
            o.zero(self.scores)
            o.zero(p.frames)
            p.frames[:, 0] = 1  # the start row (pianoroll.pianoroll_arrays)
            if held:
                self._load_held(given, hold)
            for i in range(1, length):
                self._runner.run((i, tau, mode, thr, True) if held else (i, tau, mode, thr),
                                 lambda: self._position(i, tau, mode, thr, held), lane=held)
                p.t = i
            roll = self.roll[:, : length - 1, : self.P].cpu().numpy()
            scores = self.scores.cpu().numpy()
            self._read_held(held)
        self.positions = length - 1
        return roll, scores


class TokenSampling(_Sampler):
    """Sampling for the token ends with a temperature, a top-k and a nucleus cut, the whole position on the device: the decode step of
    position i up to its logits and mst_token_step — which cuts, draws, writes the token where the next position's embedding reads it
    and keeps the sampler's books (finished sequences, scores, the `active` counter) — are ONE captured graph per position. The draw's
    seed is a device word the host rewrites before a run, so the graphs captured by one run replay for every later one. (The draw forms
    both softmaxes itself: these graphs have no softmax_ce launch.) tau, top_k and top_p are launch constants of mst_token_step: a
    graph is kept per (position, tau, top_k, top_p).

    Constrained runs (run(..., given, hold)) end every position's graph in mst_token_step_held instead: a held position writes the
    given token, the others draw as ever. As in FrameSampling the mask and the piece are device buffers of the sampler, the graph key
    gains one boolean, and the held tokens' summed -log p is left in self.held_scores (host fp32 [N])."""

    def __init__(self, store, N, L, attention="query", keep_logits=False):
        """L positions: the start row + up to L - 1 tokens. keep_logits: every position's logits stay in self.logits (fp32 [N, L, V],
        row i = what position i's draw read; tests and diagnostics)"""
        cfg = store.cfg
        if cfg.kind != "token":
            raise ValueError("TokenSampling draws tokens; the piano-roll ends have FrameSampling")
        if L < 2:
            raise ValueError("TokenSampling needs at least two positions")
        self.N, self.L, self.V = N, L, cfg.out_dim
        self.plan = DecodePlan(store, N, L, attention=attention)
        dev = store.device
        self.seqs = torch.zeros(N, L, dtype=torch.int32, device=dev)
        self.scores = torch.zeros(N, dtype=torch.float32, device=dev)
        self.active = torch.zeros(L + 1, dtype=torch.int32, device=dev)
        self.logits = torch.zeros(N, L, self.V, dtype=torch.float32, device=dev) if keep_logits else None
        self._seed_words(dev)
        self._runner = PositionGraphs(self.plan, capture_behind=True)
        self._graphs = self._runner.graphs  # (position, tau, top_k, top_p[, True: constrained]) -> ops.Graph
        self.positions = 0
        self.given = self.hold = self.held_dev = None  # device buffers of constrained runs, allocated by the first one
        self.held_scores = None                        # host fp32 [N] of the latest constrained run

    def _position(self, i, tau, top_k, top_p, held=False):
        p = self.plan
        p._position(i, probs=False)
        if self.logits is not None:
            self.logits[:, i].copy_(p.logits[:, : self.V])  # (a device copy: part of the position's graph)
        if held:
            o.token_step_held(p.logits, self.V, i, self.seed_word, self.seqs, self.scores, p.tokens, self.eos, self.pad, self.given, self.hold,
                              self.held_dev, tau=tau, top_k=top_k, top_p=top_p, active=self.active)
        else:
            o.token_step(p.logits, self.V, i, self.seed_word, self.seqs, self.scores, p.tokens, self.eos, self.pad, tau=tau, top_k=top_k,
                         top_p=top_p, active=self.active)

    def _constraint(self, given, hold, length):
        """host copies of (given int32, hold uint8) as [N, T], T <= length, in the sequence's indexing (index 0 is SOS and never held)"""
        if given is None or hold is None:
            raise ValueError("a constrained run needs both `given` and `hold`")
        given, hold = np.asarray(given), np.asarray(hold)
        if given.shape != hold.shape or given.ndim != 2 or given.shape[0] != self.N:
            raise ValueError(f"given and hold must both be [{self.N}, tokens], got {given.shape} and {hold.shape}")
        if given.shape[1] > length:
            raise ValueError(f"{given.shape[1]} constrained tokens for a run of {length}")
        hold = (hold != 0).astype(np.uint8)
        hold[:, :1] = 0
        bad = (hold != 0) & ((given < 0) | (given >= self.V))
        if bad.any():
            raise ValueError(f"a held token outside [0, {self.V}): {np.asarray(given)[bad][:8].tolist()}")
        return np.where(hold != 0, given, self.pad).astype(np.int32), hold

    def _held_buffers(self):
        return torch.zeros_like(self.seqs), torch.zeros(self.N, self.L, dtype=torch.uint8, device=self.seqs.device)

    def _load_constraint(self, given, hold):
        T = given.shape[1]
        o.zero(self.hold)  # (positions behind T hold nothing)
        self.given[:, :T].copy_(torch.from_numpy(given))
        self.hold[:, :T].copy_(torch.from_numpy(hold))

    def run(self, row0, length=None, tau=1.0, top_k=0, top_p=1.0, seed=0, check_every=8, given=None, hold=None):
        """row0: [N, >= D] initial decoder rows. Decodes positions 1 .. length - 1 (default: all L - 1), stopping early once every
        sequence has ended (looked at every check_every positions), and returns (token rows [N, n] int32, scores [N]) as host arrays.
        given, hold: host arrays [N, T <= length] in the returned rows' indexing: token [n, i] is given[n, i] where hold[n, i] != 0
        (i >= 1) and drawn elsewhere; the scores then sum the drawn tokens only, and the held tokens' cost is left in
        self.held_scores. A run does not stop before its last held position."""
        length = self._run_length(length)
        tau, top_k, top_p = float(tau), int(top_k), float(top_p)
        if not (0.0 < tau < float("inf")) or top_k < 0 or not 0.0 < top_p <= 1.0:
            raise ValueError(f"tau > 0 finite, top_k >= 0 and 0 < top_p <= 1 wanted, got {tau}, {top_k}, {top_p}")
        held, last_held = given is not None or hold is not None, 0
        if held:
            given, hold = self._constraint(given, hold, length)
            cols = np.nonzero(hold.any(0))[0]
            last_held = int(cols[-1]) if cols.size else 0
        with self._started(row0, seed) as p:
            self._sos_rows(self.seqs, self.scores)
            o.zero(self.active)
            p.tokens.fill_(self.sos)
            if held:
                self._load_held(given, hold)
            last = 0
            for i in range(1, length):
                self._runner.run((i, tau, top_k, top_p, True) if held else (i, tau, top_k, top_p),
                                 lambda: self._position(i, tau, top_k, top_p, held), lane=held)
                p.t = last = i
                if i % check_every == 0 and i >= last_held and int(self.active[i].item()) == 0:
                    break
            seqs = self.seqs[:, : last + 1].cpu().numpy()
            scores = self.scores.cpu().numpy()
            self._read_held(held)
        self.positions = last
        return seqs, scores
