"""Time bench.py's captured training step with clipping by the global gradient norm off (the default) and on, in one process,
alternating the two in rounds, HIP events around every replay. Prints one JSON line.

    python tools/bench_clip.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4] [--max-norm 1.0]

Same inputs, weights, dropout and step options as bench.py's resident-data run of that config. "on" issues one launch more, the sum of
squares of the gradient bucket (mst_grad_sumsq), and the optimizer launch in its gnorm form. For a kernel timeline of either
step run one mode alone under a kernel trace (--modes on --rounds 1) and read it with tools/step_timeline.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(bench.CONFIGS), default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per mode and round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--modes", default="off,on", help="which steps to build (one alone: for a profiler run)")
    ap.add_argument("--max-norm", type=float, default=1.0, help="clip_global_norm of the 'on' step")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py needs an MI355X: the training step has no CPU fallback")
    from musicstyletransfer_amd import engine as E
    from musicstyletransfer_amd import ops as o
    c = bench.CONFIGS[a.config]
    B, T, P = c["B"], c["T"], c["P"]
    dev = torch.device("cuda", 0)
    adt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float16
    host = bench.synthetic_batches(1, B, T, P, seed=1234)[0]
    stream = torch.cuda.Stream()
    plans = {}
    with torch.cuda.stream(stream):
        for mode in a.modes.split(","):
            cfg = E.VAEConfig(e_dropout=bench.DROPOUT, d_dropout=bench.DROPOUT, **bench.model_dims(c))
            store = E.ParamStore(cfg, dev, adt, seed=1234)
            store.tail_policy = "raise"
            plan = E.StepPlan(store, B, T, lr=3e-4, clip_gradient=1.0, kl_weight=1.0, global_batch=B, internal_eps=True, seed=1000,
                              **(dict(clip_global_norm=a.max_norm) if mode == "on" else {}))
            assert plan.forms.gnorm == (mode == "on")
            plan.bind_inputs(plan.pack_batch(host["x"], host["seq_lens"], host["classes"], host["labels"]).to(dev))
            plan.step_kernels(True)  # eager first (module loads), then capture
            torch.cuda.synchronize()
            plan.capture(True)
            for _ in range(a.warmup):
                plan.run()
            torch.cuda.synchronize()
            plans[mode] = (store, plan)
        times = {m: [] for m in plans}
        for _ in range(a.rounds):
            for mode, (store, plan) in plans.items():
                ev = [o.Event() for _ in range(a.steps + 1)]
                ev[0].record()
                for i in range(a.steps):
                    plan.run()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                times[mode] += [ev[i].elapsed_ms(ev[i + 1]) for i in range(a.steps)]
        extra = {}
        for mode, (store, plan) in plans.items():
            m = store.read_metrics(reset=False)
            assert m["skipped_steps"] == 0, mode
            assert torch.isfinite(plan.total).all(), mode
            extra[f"{mode}_kernel_nodes"] = plan.graph_nodes()[1]
            if mode == "on":
                assert m["nonfinite_steps"] == 0 and m["grad_norm"] > 0
                extra.update(on_steps=int(store.step_state[0].item()), on_grad_norm=round(m["grad_norm"], 6),
                             on_grad_norm_max=round(m["grad_norm_max"], 6), on_clip_frac=round(m["clip_frac"], 4))
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for m, v in times.items()}
    # per-round medians: the spread of a mode against itself is the yardstick for the difference between the two
    rounds = {m: [round(sorted(v[r * a.steps:(r + 1) * a.steps])[a.steps // 2], 4) for r in range(a.rounds)] for m, v in times.items()}
    line = dict(config=a.config, name=c["name"], steps_per_mode=a.steps * a.rounds, rounds=a.rounds, max_norm=a.max_norm,
                **{f"{m}_ms_per_step": round(t, 4) for m, t in med.items()}, p10_p90_ms=spread, round_medians_ms=rounds, **extra)
    if "off" in med and "on" in med:
        line["on_over_off"] = round(med["on"] / med["off"], 4)
        line["on_minus_off_us"] = round(1e3 * (med["on"] - med["off"]), 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
