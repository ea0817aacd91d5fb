"""Time one posterior draw of the importance-weighted bound (engine.IWBound): the replayed DRAW PASS — bookkeeping, latent
launch, decoder layers, output layer, plain loss, mst_iw_fold — against a FULL inference forward of the same plan scored and folded the
same way, which is what a draw would cost without the decoder-only pass. Both are captured graphs, replayed in alternating rounds
with HIP events around every replay; one process, one plan per shape. Prints one JSON line.

    python tools/bench_iw.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4] [--samples 16]

Shapes: bench.py's configs[--config] (resident synthetic batch, bench.py's weights) and the piano-roll shape of tests/test_iw_gpu.py
(P 128, encoder 64 x 2, decoder 128 x 1, B 4, T 64). Also reported: the kernel launches of either graph, and the wall time of whole
IWBound.run(--samples) calls (one full forward + samples - 1 replays + mst_iw_finish, host-synchronised), per draw."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEST_SHAPE = dict(name="test-roll-d128", dims=("pianoroll", 128, 128, 2, 32, 64, 2, 4, 128, 1, 4), B=4, T=64, dtype="bf16")


def measure(a, name, cfg, B, T, adt, host):
    import numpy as np
    import torch
    from musicstyletransfer_amd import engine as E
    from musicstyletransfer_amd import ops as o
    dev = torch.device("cuda", 0)
    store = E.ParamStore(cfg, dev, adt, seed=1234)
    Z = cfg.latent_dim
    with torch.no_grad():  # keep sigma off 0 (tests/test_step_gpu.py: _setup), so that every draw counts
        store.p("encoder.latent_proj.weight")[Z:].mul_(0.25)
        store.p("encoder.latent_proj.bias")[Z:].add_(1.5)
    store.refresh_shadows()
    plan = E.StepPlan(store, B, T, internal_eps=True)
    plan.bind_inputs(plan.pack_batch(host["x"], host["seq_lens"], host["classes"], host["labels"]).to(dev))
    iw = E.IWBound(plan)

    def full_pass():
        plan.forward(inference=True)
        iw._score()

    with torch.cuda.stream(iw.stream):
        o.zero(iw.state)
        full_pass()      # eager first (module loads), then capture
        iw.draw_pass()
        torch.cuda.synchronize()
        graphs = {"full": o.Graph().capture(full_pass), "draw": o.Graph().capture(iw.draw_pass)}
        for g in graphs.values():
            for _ in range(a.warmup):
                g.launch()
        torch.cuda.synchronize()
        times = {m: [] for m in graphs}
        for _ in range(a.rounds):
            for mode, g in graphs.items():
                ev = [o.Event() for _ in range(a.steps + 1)]
                ev[0].record()
                for i in range(a.steps):
                    g.launch()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                times[mode] += [ev[i].elapsed_ms(ev[i + 1]) for i in range(a.steps)]
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    rounds = {m: [round(sorted(v[r * a.steps:(r + 1) * a.steps])[a.steps // 2], 4) for r in range(a.rounds)] for m, v in times.items()}
    out = dict(name=name, B=B, T=T, forms=dict(riders=plan.forms.riders, tails=plan.forms.tails, fuse_bce=plan.forms.fuse_bce),
               full_kernel_nodes=graphs["full"].kernel_nodes, draw_kernel_nodes=graphs["draw"].kernel_nodes,
               full_us=round(1e3 * med["full"], 2), draw_us=round(1e3 * med["draw"], 2), draw_over_full=round(med["draw"] / med["full"], 4),
               p10_p90_us={m: [round(1e3 * sorted(v)[len(v) // 10], 2), round(1e3 * sorted(v)[(9 * len(v)) // 10], 2)] for m, v in times.items()},
               round_medians_ms=rounds)
    # whole runs, as the trainer and generate.py issue them
    iw.run(a.samples)
    torch.cuda.synchronize()
    walls = []
    for _ in range(max(3, a.rounds)):
        t0 = time.perf_counter()
        iw.run(a.samples)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    res = iw.results()
    assert res["valid"].all() and np.isfinite(res["log_px"]).all(), name
    s = E.iw_scores(iw.read_acc(), iw.cells)
    out.update(samples=a.samples, run_wall_us_per_draw=round(1e6 * sorted(walls)[len(walls) // 2] / a.samples, 2), captures=iw.captures,
               iw_gap=round(s["iw_gap"], 4), iw_ess=round(s["iw_ess"], 4), iw_bits_per_cell=round(s["iw_bits_per_cell"], 6))
    return out


def main(argv=None):
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(bench.CONFIGS), default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed replays per graph and round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--samples", type=int, default=16, help="K of the whole-run timing")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_iw.py needs an MI355X: the forward pass has no CPU fallback")
    from musicstyletransfer_amd import engine as E
    c = bench.CONFIGS[a.config]
    shapes = [(c["name"], E.VAEConfig(**bench.model_dims(c)), c["B"], c["T"], c["dtype"], c["P"]),
              (TEST_SHAPE["name"], E.VAEConfig(*TEST_SHAPE["dims"]), TEST_SHAPE["B"], TEST_SHAPE["T"], TEST_SHAPE["dtype"], TEST_SHAPE["dims"][1])]
    line = dict(config=a.config, replays_per_graph=a.steps * a.rounds, rounds=a.rounds, shapes=[])
    for name, cfg, B, T, dtype, P in shapes:
        host = bench.synthetic_batches(1, B, T, P, seed=1234)[0]
        line["shapes"].append(measure(a, name, cfg, B, T, torch.bfloat16 if dtype == "bf16" else torch.float16, host))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
