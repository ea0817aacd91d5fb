"""Time bench.py's captured training step with the exponential moving average of the weights off (the default) and on, in one process,
alternating the two in rounds, HIP events around every replay. Prints one JSON line.

    python tools/bench_ema.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4] [--decay 0.999]

Same inputs, weights, dropout and step options as bench.py's resident-data run of that config. "on" issues the same launches in the same
order, with the optimizer launch(es) in the averaging form (mst_adam_args.ema: one more fp32 read and one more fp32 write of the bucket;
DESIGN §13). For a kernel timeline of either step run one mode alone under a kernel trace (--modes on --rounds 1) and read it with
tools/step_timeline.py."""
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
    ap.add_argument("--decay", type=float, default=0.999, help="ema_decay of the 'on' step")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py needs an MI355X: the training step has no CPU fallback")
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
                              **(dict(ema_decay=a.decay) if mode == "on" else {}))
            assert plan.forms.ema == (mode == "on") and (store.ema is not None) == (mode == "on")
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
        extra = dict(bucket_floats=next(iter(plans.values()))[0].n)
        for mode, (store, plan) in plans.items():
            m = store.read_metrics(reset=False)
            assert m["skipped_steps"] == 0 and m["nonfinite_steps"] == 0, mode
            assert torch.isfinite(plan.total).all(), mode
            extra[f"{mode}_nodes"], extra[f"{mode}_kernel_nodes"] = plan.graph_nodes()
            if mode == "on":
                assert torch.isfinite(store.ema).all() and not torch.equal(store.ema, store.w)
                extra.update(on_steps=int(store.step_state[0].item()),
                             on_ema_minus_w_rms=round(float((store.ema - store.w).double().pow(2).mean().sqrt()), 8))
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for m, v in times.items()}
    # per-round medians: the spread of a mode against itself is the yardstick for the difference between the two
    rounds = {m: [round(sorted(v[r * a.steps:(r + 1) * a.steps])[a.steps // 2], 4) for r in range(a.rounds)] for m, v in times.items()}
    line = dict(config=a.config, name=c["name"], steps_per_mode=a.steps * a.rounds, rounds=a.rounds, decay=a.decay,
                **{f"{m}_ms_per_step": round(t, 4) for m, t in med.items()}, p10_p90_ms=spread, round_medians_ms=rounds, **extra)
    if "off" in med and "on" in med:
        line["on_over_off"] = round(med["on"] / med["off"], 4)
        line["on_minus_off_us"] = round(1e3 * (med["on"] - med["off"]), 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
