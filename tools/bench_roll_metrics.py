"""Time bench.py's captured training step with the piano-roll counts off (bench.py's own step) and on (the trainer's default for
piano-roll models), in one process, alternating the two in rounds, HIP events around every replay. Prints one JSON line.

    python tools/bench_roll_metrics.py [--config 1] [--steps 200] [--warmup 20] [--rounds 4]

Same inputs, weights, dropout and step options as bench.py's resident-data run of that config. "on" issues the same launches in the same
order; the launch that computes the BCE (mst_dec_tail_step at configs[1], mst_sigmoid_bce_counts at configs[2]) also counts tp / pred /
pos / cells into ParamStore.roll_counts. For a kernel timeline of either step run one mode alone under a kernel trace
(--modes on --rounds 1) and read it with tools/step_timeline.py."""
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
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_roll_metrics.py needs an MI355X: the training step has no CPU fallback")
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
            if cfg.kind != "pianoroll":
                raise SystemExit(f"config {a.config} has token ends: there is nothing to count")
            store = E.ParamStore(cfg, dev, adt, seed=1234)
            store.tail_policy = "raise"
            plan = E.StepPlan(store, B, T, lr=3e-4, clip_gradient=1.0, kl_weight=1.0, global_batch=B, internal_eps=True, seed=1000)
            plan.track_roll_metrics = mode == "on"
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
            assert m["skipped_steps"] == 0 and m["nonfinite_steps"] == 0, mode
            assert torch.isfinite(plan.total).all(), mode
            extra[f"{mode}_nodes"], extra[f"{mode}_kernel_nodes"] = plan.graph_nodes()
            F = plan.forms
            extra[f"{mode}_route"] = "dec_tail_step" if F.fuse_bce and F.dec_tail else "gemm_sigmoid_bce" if F.fuse_bce else "sigmoid_bce"
            steps = 1 + a.warmup + a.steps * a.rounds
            if mode == "on":  # every step counted every cell; the labels never change
                assert m["roll_cells"] == steps * B * T * P, m
                extra.update(on_steps=steps, **{k: m[k] for k in ("roll_tp", "roll_pred", "roll_pos", "roll_cells")},
                             **{k: round(v, 6) for k, v in E.roll_scores(m["roll_tp"], m["roll_pred"], m["roll_pos"], m["roll_cells"]).items()})
            else:
                assert m["roll_cells"] == 0, m
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: [round(sorted(v)[len(v) // 10], 4), round(sorted(v)[(9 * len(v)) // 10], 4)] for m, v in times.items()}
    # per-round medians: the spread of a mode against itself is the yardstick for the difference between the two
    rounds = {m: [round(sorted(v[r * a.steps:(r + 1) * a.steps])[a.steps // 2], 4) for r in range(a.rounds)] for m, v in times.items()}
    line = dict(config=a.config, name=c["name"], steps_per_mode=a.steps * a.rounds, rounds=a.rounds,
                **{f"{m}_ms_per_step": round(t, 4) for m, t in med.items()}, p10_p90_ms=spread, round_medians_ms=rounds, **extra)
    if "off" in med and "on" in med:
        line["on_over_off"] = round(med["on"] / med["off"], 4)
        line["on_minus_off_us"] = round(1e3 * (med["on"] - med["off"]), 2)
        line["off_round_spread_us"] = round(1e3 * (max(rounds["off"]) - min(rounds["off"])), 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
