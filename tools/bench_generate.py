"""Timings of latent-space generation on the configs[1] decoder (B 64, T 256 -> 512 positions, P 128, bf16), in ONE process:

  1. the piano-roll host loop of Sampling.sample (per position: a device->host copy of the probabilities, a numpy Bernoulli draw, a
     host->device copy of the frame) against decode.FrameSampling after its graphs are captured (the draw inside each position's
     graph, one copy at the end) — per decoded position;
  2. the restyle of one batch to both classes: what Sampling.process_batch runs in front of its decode loops (one full inference
     forward per class) against what LatentGenerator.transfer runs (one encode + one mst_latent_rows launch for all rows).

    python tools/bench_generate.py [--reps 3] [--out FILE]

Every timed window ends in a device synchronise; the two forms of each pair alternate inside the process; the first pass of
every shape (lazy module loads, plan construction, graph capture) is outside the timed windows. Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "bench_generate needs a GPU"
    from musicstyletransfer_amd import generate as G
    from musicstyletransfer_amd.VarAutoEncoder import model, sampler as S
    from musicstyletransfer_amd.VarAutoEncoder.data import Batch
    from musicstyletransfer_amd.VarAutoEncoder.transformer import TransformerConfig
    from musicstyletransfer_amd.VarAutoEncoder.utils import gpu

    B, T, P, Z = args.batch, args.frames, 128, 64
    cfg = model.ModelConfig(model.EncoderConfig(TransformerConfig(256, 0.2, 2, 8, P), Z, 2, P),
                            model.DecoderConfig(TransformerConfig(128, 0.2, 1, 8, P), Z, 2, P), kind="pianoroll")
    m = model.Model(cfg).initialize(gpu(0), seed=1234)
    rng = np.random.default_rng(0)
    x = (rng.random((B, T, P)) < 0.04).astype(np.uint8)
    x[:, 0] = 0
    x[:, 0, 0] = 1
    batch = Batch([x, np.full(B, T, np.int64), rng.integers(0, 2, B)], [])
    positions = 2 * T - 1  # decoded positions of one sample() call (sampler.py:163)

    host = S.Sampling(seed=1)
    host.update_parameters(m)
    dev = S.Sampling(seed=1, frames_on_device=True)
    dev.update_parameters(m)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # warm-up: every shape once (module loads, plan construction, graph capture), then one replay of the device loop
    host.sample(batch)
    dev.sample(batch)
    dev.sample(batch)
    fs = m.frame_sampling_plan(B, 2 * T, host.attention)
    row0 = m.decoder.initial_rows(*batch.data)
    t_host, t_dev, t_loop = [], [], []
    for _ in range(args.reps):
        t_host.append(timed(lambda: host.sample(batch)))
        t_dev.append(timed(lambda: dev.sample(batch)))
        t_loop.append(timed(lambda: fs.run(row0, seed=3)))  # the device loop alone (row 0 given)

    # restyle to both classes: what runs in front of the decode loop
    gen = G.LatentGenerator(m, decoder="sampling")
    rec = G.recipe_transfer(B, [0, 1])
    classes = np.asarray(batch.data[2])

    def two_forwards():
        for c in range(2):
            m.decoder.initial_rows(batch.data[0], batch.data[1], np.full_like(classes, c))

    def one_encode():
        mu, _ = gen.encode(batch)
        gen._rows(rec, mu, None, 0, len(rec))

    two_forwards()
    one_encode()
    t_two, t_one = [], []
    for _ in range(max(args.reps, 7)):
        t_two.append(timed(two_forwards))
        t_one.append(timed(one_encode))

    med = lambda v: float(np.median(v))
    res = dict(bench="generate", B=B, T=T, P=P, positions=positions, reps=args.reps,
               host_loop_us_per_position=med(t_host) / positions * 1e6, host_loop_s=t_host,
               frame_sampling_us_per_position=med(t_dev) / positions * 1e6, frame_sampling_s=t_dev,
               frame_sampling_loop_only_us_per_position=med(t_loop) / positions * 1e6,
               restyle_two_forwards_ms=med(t_two) * 1e3, restyle_two_forwards_all_ms=[t * 1e3 for t in t_two],
               restyle_one_encode_ms=med(t_one) * 1e3, restyle_one_encode_all_ms=[t * 1e3 for t in t_one],
               graphs_captured=len(fs._graphs))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
