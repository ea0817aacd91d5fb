"""Time bench.py's captured training step with the decoder non-causal (the default) and causal (VAEConfig.d_causal), in one
process, alternating the two in rounds, HIP events around every replay. Prints one JSON line.

    python tools/bench_causal.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4]

Same inputs, weights, dropout and step options as bench.py's resident-data run of that config. The two steps differ only in
the decoder's attention launches (attention_fwd.hip / attention_bwd.hip vs attention_causal.hip) and, in the causal one, a projection GEMM where a
decoder layer other than the first takes the fused projection + attention launch."""
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
    ap.add_argument("--modes", default="default,causal", help="which steps to build (one alone: for a profiler run)")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_causal.py needs an MI355X: the training step has no CPU fallback")
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
            cfg = E.VAEConfig(e_dropout=bench.DROPOUT, d_dropout=bench.DROPOUT, d_causal=mode == "causal", **bench.model_dims(c))
            store = E.ParamStore(cfg, dev, adt, seed=1234)
            store.tail_policy = "raise"
            plan = E.StepPlan(store, B, T, lr=3e-4, clip_gradient=1.0, kl_weight=1.0, global_batch=B, internal_eps=True, seed=1000)
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
        for mode, (store, plan) in plans.items():
            assert store.read_metrics(reset=False)["skipped_steps"] == 0, mode
            assert torch.isfinite(plan.total).all(), mode
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for m, v in times.items()}
    line = dict(config=a.config, name=c["name"], steps_per_mode=a.steps * a.rounds, rounds=a.rounds,
                **{f"{m}_ms_per_step": round(t, 4) for m, t in med.items()}, p10_p90_ms=spread)
    if "default" in med and "causal" in med:
        line["causal_over_default"] = round(med["causal"] / med["default"], 4)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
