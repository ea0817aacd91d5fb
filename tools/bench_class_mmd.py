"""Time bench.py's captured training step with the class-conditional MMD penalty off (bench.py's own step) and on (--class-mmd),
in one process, alternating the two in rounds, HIP events around every replay — once with the off step built first and once with
the on step built first (which store was allocated and captured first has moved such differences before). Prints one JSON line.

    python tools/bench_class_mmd.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4] [--lam 100]

Same inputs, weights, dropout and step options as bench.py's resident-data run of that config. "on" issues the same launches in the same
order plus one, mst_class_mmd, directly behind the latent block's backward launch: one kernel node more. For a kernel
timeline of either step run one mode alone under a kernel trace (--orders on --rounds 1) and read it with tools/step_timeline.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a, bench, modes):
    """build the steps of `modes` in that order, then time them in alternating rounds -> dict of figures"""
    import torch
    from musicstyletransfer_amd import engine as E
    from musicstyletransfer_amd import ops as o
    c = bench.CONFIGS[a.config]
    B, T, P = c["B"], c["T"], c["P"]
    dev = torch.device("cuda", 0)
    adt = torch.bfloat16 if c["dtype"] == "bf16" else torch.float16
    host = bench.synthetic_batches(1, B, T, P, seed=1234)[0]
    plans = {}
    for mode in modes:
        cfg = E.VAEConfig(e_dropout=bench.DROPOUT, d_dropout=bench.DROPOUT, **bench.model_dims(c))
        store = E.ParamStore(cfg, dev, adt, seed=1234)
        store.tail_policy = "raise"
        plan = E.StepPlan(store, B, T, lr=3e-4, clip_gradient=1.0, kl_weight=1.0, global_batch=B, internal_eps=True, seed=1000)
        plan.class_mmd = a.lam if mode == "on" else 0.0
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
    out = {}
    for mode, (store, plan) in plans.items():
        m = store.read_metrics(reset=False)
        assert m["skipped_steps"] == 0 and m["nonfinite_steps"] == 0, mode
        assert torch.isfinite(plan.total).all(), mode
        out[f"{mode}_nodes"], out[f"{mode}_kernel_nodes"] = plan.graph_nodes()
        steps = 1 + a.warmup + a.steps * a.rounds
        acc = m["class_mmd_acc"]
        if mode == "on":  # every step counted one launch
            assert acc[1] + acc[2] == steps and plan.class_mmd_issued == "grad", acc
            s = E.class_mmd_score(acc)
            out.update(on_steps=steps, class_mmd=round(s["class_mmd"], 8), class_mmd_bad=s["class_mmd_bad"])
        else:
            assert not acc.any() and plan.class_mmd_issued is None, mode
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    # per-round medians: the spread of a mode against itself is the yardstick for the difference between the two
    rounds = {m: [round(sorted(v[r * a.steps:(r + 1) * a.steps])[a.steps // 2], 4) for r in range(a.rounds)] for m, v in times.items()}
    out.update({f"{m}_ms_per_step": round(t, 4) for m, t in med.items()},
               p10_p90_ms={m: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for m, v in times.items()},
               round_medians_ms=rounds)
    if "off" in med and "on" in med:
        out["on_over_off"] = round(med["on"] / med["off"], 4)
        out["on_minus_off_us"] = round(1e3 * (med["on"] - med["off"]), 2)
        out["off_round_spread_us"] = round(1e3 * (max(rounds["off"]) - min(rounds["off"])), 2)
    return out


def main(argv=None):
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, choices=sorted(bench.CONFIGS), default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps per mode and round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--lam", type=float, default=100.0, help="the penalty's multiplier in the on mode")
    ap.add_argument("--orders", default="off,on;on,off", help="build orders, ';' between them (one mode alone: for a profiler run)")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_class_mmd.py needs an MI355X: the training step has no CPU fallback")
    c = bench.CONFIGS[a.config]
    line = dict(config=a.config, name=c["name"], steps_per_mode=a.steps * a.rounds, rounds=a.rounds, lam=a.lam)
    with torch.cuda.stream(torch.cuda.Stream()):
        for order in a.orders.split(";"):
            line["built_" + "_then_".join(order.split(","))] = measure(a, bench, order.split(","))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
