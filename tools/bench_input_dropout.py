"""Time bench.py's captured training step with decoder-input dropout off (the default) and on, in one process, alternating the two in
rounds, HIP events around every replay. Prints one JSON line.

    python tools/bench_input_dropout.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4] [--p 0.25] [--modes off,on]

Same inputs, weights, layer dropout and step options as bench.py's resident-data run of that config. "on" draws the keep mask and writes
the masked copy of the frames in the step's bookkeeping, which then is a launch of its own in front of the embedding GEMMs instead of
workgroups of that launch (piano-roll ends: one kernel node more). --modes off alone also runs on a tree from before the
option existed: the off step against that tree's step is the "nothing moved" measurement."""
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
    ap.add_argument("--modes", default="off,on", help="which steps to build (one alone: for a profiler run, or an older tree)")
    ap.add_argument("--p", type=float, default=0.25, help="d_input_dropout of the 'on' step")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_dropout.py needs an MI355X: the training step has no CPU fallback")
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
                              **(dict(d_input_dropout=a.p) if mode == "on" else {}))
            plan.bind_inputs(plan.pack_batch(host["x"], host["seq_lens"], host["classes"], host["labels"]).to(dev))
            plan.step_kernels(True)  # eager first (module loads), then capture
            assert getattr(plan.forms, "in_drop", False) == (mode == "on")  # (resolved by the training step's forward())
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
            assert m["skipped_steps"] == 0 and m["nonfinite_steps"] == 0, mode
            assert torch.isfinite(plan.total).all(), mode
            nodes, kernels = plan.graph_nodes()
            extra[f"{mode}_graph_nodes"], extra[f"{mode}_kernel_nodes"] = nodes, kernels
            if mode == "on":
                extra.update(on_steps=int(store.step_state[0].item()), on_kept_last_step=round(float(plan.in_keep.float().mean().item()), 4))
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for m, v in times.items()}
    # per-round medians: the spread of a mode against itself is the yardstick for the difference between the two
    rounds = {m: [round(sorted(v[r * a.steps:(r + 1) * a.steps])[a.steps // 2], 4) for r in range(a.rounds)] for m, v in times.items()}
    line = dict(config=a.config, name=c["name"], steps_per_mode=a.steps * a.rounds, rounds=a.rounds, p=a.p,
                **{f"{m}_ms_per_step": round(t, 4) for m, t in med.items()}, p10_p90_ms=spread, round_medians_ms=rounds, **extra)
    if "off" in med and "on" in med:
        line["on_over_off"] = round(med["on"] / med["off"], 4)
        line["on_minus_off_us"] = round(1e3 * (med["on"] - med["off"]), 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
