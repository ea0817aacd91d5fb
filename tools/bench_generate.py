"""Timings of latent-space generation on the configs[1] decoder (B 64, T 256 -> 512 positions, P 128, bf16), in ONE process:

  1. the piano-roll host loop of Sampling.sample (per position: a device->host copy of the probabilities, a numpy Bernoulli draw, a
     host->device copy of the frame) against decode.FrameSampling after its graphs are captured (the draw inside each position's
     graph, one copy at the end) — per decoded position;
  2. the restyle of one batch to both classes: what Sampling.process_batch runs in front of its decode loops (one full inference
     forward per class) against what LatentGenerator.transfer runs (one encode + one mst_latent_rows launch for all rows).

  3. (--case token) the token ends' draw on a token model of the scripts/train-vae.sh shape (V 293, encoder 256 x 2 x 8, decoder
     128 x 1 x 8, latent 256, B 64, 129 decoded positions): decode.AncestralSampling (eager launches: the decode step, a softmax and
     mst_sample_step per position) against decode.TokenSampling (one graph replay per position: the decode step and mst_token_step)
     with the filters off and with top_k 40, top_p 0.9 — per decoded position, row 0 given.

  4. (--case held, and part of --case pianoroll) constrained decoding: decode.FrameSampling's loop with HALF the cells held (a random
     mask and piece; every position's graph ends in mst_frame_step_held, which reads two more bytes per cell) beside the
     unconstrained loop of the same sampler — per decoded position, row 0 given, the two alternating.

    python tools/bench_generate.py [--case all|pianoroll|token|held] [--reps 3] [--out FILE]

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


def token_case(args):
    """-> dict of the token ends' timings (medians over max(reps, 7) windows per form, the forms alternating)"""
    import torch
    from musicstyletransfer_amd import decode
    from musicstyletransfer_amd.MIDIUtil.defaults import NUM_EVENTS
    from musicstyletransfer_amd.VarAutoEncoder import model
    from musicstyletransfer_amd.VarAutoEncoder.transformer import TransformerConfig
    from musicstyletransfer_amd.VarAutoEncoder.utils import gpu

    B, T, V, Z = args.batch, 65, NUM_EVENTS, 256
    cfg = model.ModelConfig(model.EncoderConfig(TransformerConfig(256, 0.2, 2, 8, V), Z, 2, V),
                            model.DecoderConfig(TransformerConfig(128, 0.2, 1, 8, V), Z, 2, V))
    m = model.Model(cfg).initialize(gpu(0), seed=1234)
    rng = np.random.default_rng(0)
    tokens = rng.integers(3, V, (B, T))
    tokens[:, 0] = 1
    row0 = m.decoder.initial_rows(tokens, np.full(B, T, np.int64), rng.integers(0, 2, B))
    i_max = 2 * T  # sampler.py:163: 129 decoded positions
    anc = decode.AncestralSampling(m.store, B, i_max, seed=1)
    tok = decode.TokenSampling(m.store, B, i_max)
    forms = {"ancestral": lambda: anc.run(row0),
             "token_sampling_filters_off": lambda: tok.run(row0, seed=3),
             "token_sampling_top_k40_top_p0.9": lambda: tok.run(row0, top_k=40, top_p=0.9, seed=3)}
    who = {"ancestral": anc, "token_sampling_filters_off": tok, "token_sampling_top_k40_top_p0.9": tok}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for fn in forms.values():  # module loads, graph capture, then one replay
        fn()
        fn()
    per = {k: [] for k in forms}
    for _ in range(max(args.reps, 7)):
        for k, fn in forms.items():
            t = timed(fn)
            per[k].append(t / max(1, who[k].positions) * 1e6)
    res = dict(token_B=B, token_V=V, token_positions=i_max - 1, token_graphs_captured=len(tok._graphs))
    for k, v in per.items():
        res["token_" + k + "_us_per_position"] = float(np.median(v))
        res["token_" + k + "_all_us"] = v
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--case", default="all", choices=("all", "pianoroll", "token", "held"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "bench_generate needs a GPU"
    res = dict(bench="generate", reps=args.reps)
    if args.case in ("all", "pianoroll"):
        res.update(pianoroll_case(args))
    if args.case in ("all", "token"):
        res.update(token_case(args))
    if args.case == "held":
        res.update(held_case(args))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


def _pianoroll_setup(args):
    """the configs[1] piano-roll model, one batch of it and the number of decoded positions of one sample() call (sampler.py:163)"""
    from musicstyletransfer_amd.VarAutoEncoder import model
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
    return m, batch, B, T, P, 2 * T - 1


def held_case(args, setup=None):
    """-> FrameSampling's time per position, unconstrained and with half the cells held (medians over max(reps, 7) alternated windows;
    `unconstrained_only`: a sampler without run(given, hold) — an older tree timed by the same tool — reports the first figure alone)"""
    import inspect
    import torch
    m, batch, B, T, P, positions = setup or _pianoroll_setup(args)
    fs = m.frame_sampling_plan(B, 2 * T)
    row0 = m.decoder.initial_rows(*batch.data)
    rng = np.random.default_rng(1)
    given = (rng.random((B, positions, P)) < 0.04).astype(np.uint8)
    hold = (rng.random((B, positions, P)) < 0.5).astype(np.uint8)
    forms = {"free": lambda: fs.run(row0, seed=3)}
    if "given" in inspect.signature(fs.run).parameters:
        forms["half_held"] = lambda: fs.run(row0, seed=3, given=given, hold=hold)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def upload():  # what a constrained run does once, in front of its first position: the piece and the mask to the device
        with fs.plan._enter():
            fs._load_held(given, hold)
        fs.plan._leave()

    for fn in forms.values():  # module loads, graph capture, then one replay
        fn()
        fn()
    per = {k: [] for k in forms}
    t_up = []
    for _ in range(max(args.reps, 7)):
        for k, fn in forms.items():
            per[k].append(timed(fn) / positions * 1e6)
        if "half_held" in forms:
            t_up.append(timed(upload) * 1e3)
    res = dict(held_B=B, held_P=P, held_positions=positions, held_graphs_captured=len(fs._graphs))
    if t_up:
        res.update(constraint_upload_ms_per_run=float(np.median(t_up)), constraint_upload_all_ms=t_up)
    for k, v in per.items():
        res["frame_sampling_" + k + "_us_per_position"] = float(np.median(v))
        res["frame_sampling_" + k + "_all_us"] = v
    return res


def pianoroll_case(args):
    import torch
    from musicstyletransfer_amd import generate as G
    from musicstyletransfer_amd.VarAutoEncoder import sampler as S

    setup = _pianoroll_setup(args)
    m, batch, B, T, P, positions = setup

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
    res = dict(B=B, T=T, P=P, positions=positions,
               host_loop_us_per_position=med(t_host) / positions * 1e6, host_loop_s=t_host,
               frame_sampling_us_per_position=med(t_dev) / positions * 1e6, frame_sampling_s=t_dev,
               frame_sampling_loop_only_us_per_position=med(t_loop) / positions * 1e6,
               restyle_two_forwards_ms=med(t_two) * 1e3, restyle_two_forwards_all_ms=[t * 1e3 for t in t_two],
               restyle_one_encode_ms=med(t_one) * 1e3, restyle_one_encode_all_ms=[t * 1e3 for t in t_one],
               graphs_captured=len(fs._graphs))
    res.update(held_case(args, setup))
    return res


if __name__ == "__main__":
    main()
