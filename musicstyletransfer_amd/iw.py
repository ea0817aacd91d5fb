"""IWBound: the importance-weighted bound on log p(x) from K posterior draws, run on the StepPlan it is given."""
import numpy as np
import torch

from . import ops as o
from .step_math import check_iw


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
