"""mst_token_step and decode.TokenSampling on the GPU: the kept set of the temperature / top-k / nucleus cuts EXACTLY as the fp64
reference has it (tests/token_refs.py, whose generator fits top_p to the row), the draw's distribution over the kept set, the
sampler's books, the seed word under graph replay, the captured loop on a toy token model, and that the default paths are untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_refs as T  # noqa: E402

pytestmark = pytest.mark.gpu

EOS, PAD, SOS = 2, 0, 1
_DT = {torch.bfloat16: "bf16", torch.float16: "fp16"}
CASES = [(V, d) for V in T.SAMPLE_V for d in T.DTYPES]
CASE_IDS = [f"V{V}-{_DT[d]}" for V, d in CASES]


def test_the_token_ids_are_the_packages():
    from musicstyletransfer_amd.MIDIUtil.defaults import EOS_ID, PAD_ID, SOS_ID
    assert (EOS_ID, PAD_ID, SOS_ID) == (EOS, PAD, SOS)


class Bench:
    """N sequences sharing one logit row, in a buffer of ldl = roundup8(V) + 8 whose pad columns hold the dtype's largest finite
    value (it would win every cut if it were read)"""

    def __init__(self, gpu, row16, N, L=6, i=2, finished=0):
        self.V, self.N, self.L, self.i = row16.numel(), N, L, i
        ldl = (self.V + 7) // 8 * 8 + 8
        self.logits = torch.full((N, ldl), torch.finfo(row16.dtype).max, dtype=row16.dtype, device=gpu)
        self.logits[:, : self.V] = row16.to(gpu)
        self.seed = torch.zeros(1, dtype=torch.int64, device=gpu)
        self.finished = finished
        self.gpu = gpu

    def launch(self, tau, top_k, top_p, seed=1234):
        from musicstyletransfer_amd import ops as o
        N, L, i = self.N, self.L, self.i
        self.seed.fill_(seed)
        seqs = torch.full((N, L), 7, dtype=torch.int32, device=self.gpu)
        seqs[: self.finished, i - 1] = EOS
        scores = torch.zeros(N, device=self.gpu)
        word = torch.full((N,), -7, dtype=torch.int32, device=self.gpu)
        active = torch.zeros(L + 1, dtype=torch.int32, device=self.gpu)
        kept = torch.full((N,), -7, dtype=torch.int32, device=self.gpu)
        o.token_step(self.logits, self.V, i, self.seed, seqs, scores, word, EOS, PAD, tau=tau, top_k=top_k, top_p=top_p, active=active,
                     kept_out=kept)
        torch.cuda.synchronize()
        return dict(seqs=seqs.cpu().numpy(), scores=scores.cpu().numpy(), word=word.cpu().numpy(), active=active.cpu().numpy(),
                    kept=kept.cpu().numpy())


# ====================================================================================================== 1. the kept set, exact
@pytest.mark.parametrize("V,dtype", CASES, ids=CASE_IDS)
def test_kept_set_is_the_references(gpu, V, dtype):
    """N = 4096 sequences sharing one row, for tau in {0.5, 1, 2} x top_k in {0, 1, 7, V} x top_p in {1, the generator's three}:
    kept_out is the reference's count on every sequence and every drawn token lies in the reference's kept set. Then the same with a
    tie group planted across rank 7 (nine columns holding one stored value). Exact: the generator leaves top_p at least 2 delta from
    every cumulative mass, so no fp32 rounding of a mass may move the cut, and the top-k cut is a cut on integers."""
    N = 4096
    rows = {"plain": T.make_row(V, dtype, seed=V)}
    if V > 1:
        rows["ties"] = T.plant_ties(rows["plain"], 7)
    worst = 0
    for name, row in rows.items():
        b = Bench(gpu, row, N)
        for tau in T.TAUS:
            for top_k in sorted({0, 1, 7, V}) if name == "plain" else (7,):
                ps = [1.0] + [T.fit_top_p(row, tau, top_k, t)[0] for t in (T.TARGETS if name == "plain" else (0.5,))]
                for top_p in dict.fromkeys(ps):
                    kept, _, _ = T.token_filter_ref(row, tau, top_k, top_p)
                    if top_p < 1.0:
                        assert T.margin(row, tau, top_k, top_p) >= 2.0
                    got = b.launch(tau, top_k, top_p, seed=1000 * top_k + int(10 * tau))
                    tok = got["seqs"][:, b.i]
                    case = (name, tau, top_k, top_p)
                    assert (got["kept"] == kept.sum()).all(), (case, int(kept.sum()), np.unique(got["kept"]))
                    assert ((tok >= 0) & (tok < V)).all(), case
                    assert kept[tok].all(), (case, np.unique(tok[~kept[tok]]))
                    worst = max(worst, int(kept.sum()))
    print(f"token_step kept sets V={V} {_DT[dtype]}: {len(rows)} rows, largest kept set {worst}")


# ====================================================================================================== 2. the distribution and the books
@pytest.mark.parametrize("V,dtype", CASES, ids=CASE_IDS)
def test_draws_follow_the_kept_distribution(gpu, V, dtype):
    """test_sample_step_follows_the_distribution's form: N = 16384 sequences sharing one row, an eighth of them finished; counts
    within 6 sigma (+ 1) of n s_j renormalised over the kept set and zero outside it; score = -log p[token] of the MODEL's softmax
    (temperature 1, unfiltered) at that test's tolerances (the row sum and the division are fp32); finished sequences get PAD, score
    0 and are written to `word`; active[i] exact; the other columns of seqs untouched"""
    N = 16384
    row = T.make_row(V, dtype, seed=V + 17)
    b = Bench(gpu, row, N, finished=N // 8)
    for tau, top_k, target in ((1.0, 0, None), (0.7, 7, 0.9), (2.0, 0, 0.5)):
        top_p = 1.0 if target is None else T.fit_top_p(row, tau, top_k, target)[0]
        kept, s, p = T.token_filter_ref(row, tau, top_k, top_p)
        got = b.launch(tau, top_k, top_p, seed=77)
        seqs, i, fin = got["seqs"], b.i, N // 8
        tok = seqs[:, i]
        assert (tok[:fin] == PAD).all() and (got["scores"][:fin] == 0).all()
        assert (got["kept"] == kept.sum()).all()
        live = tok[fin:]
        assert ((live >= 0) & (live < V)).all()
        n = len(live)
        counts = np.bincount(live, minlength=V).astype(np.float64)
        assert (counts[~kept] == 0).all()
        q = np.where(kept, s, 0.0)
        q /= q.sum()
        sigma = np.sqrt(n * q * (1 - q)) + 1.0
        assert (np.abs(counts - n * q) <= 6 * sigma).all(), ((tau, top_k, top_p), np.abs(counts - n * q).max())
        np.testing.assert_allclose(got["scores"][fin:], -np.log(p[live]), rtol=1e-4, atol=1e-5)
        assert np.array_equal(got["word"], tok)
        assert int(got["active"][i]) == int(((live != EOS) & (live != PAD)).sum())
        assert (got["active"][:i] == 0).all() and (got["active"][i + 1:] == 0).all()
        assert (seqs[:, :i] == 7).sum() == N * i - fin and (seqs[:, i + 1:] == 7).all()


# ====================================================================================================== 3. the seed word
def test_the_seed_is_a_device_word(gpu):
    """the same word gives the same bits on two launches, another word other draws, and a captured graph holding the launch draws
    anew when it is replayed after the word was rewritten"""
    from musicstyletransfer_amd import ops as o
    V, N = 293, 4096
    row = T.make_row(V, torch.bfloat16, seed=5)
    b = Bench(gpu, row, N)
    a1, a2, c = b.launch(1.0, 40, 1.0, seed=11), b.launch(1.0, 40, 1.0, seed=11), b.launch(1.0, 40, 1.0, seed=12)
    assert np.array_equal(a1["seqs"], a2["seqs"]) and np.array_equal(a1["scores"].view(np.uint32), a2["scores"].view(np.uint32))
    kept, sd, _ = T.token_filter_ref(row, 1.0, 40, 1.0)
    q = np.where(kept, sd, 0.0) / sd[kept].sum()
    differ = 1.0 - (q ** 2).sum()                          # two independent draws differ this often
    assert (a1["seqs"][:, b.i] != c["seqs"][:, b.i]).mean() > 0.5 * differ > 0.05
    seqs = torch.full((N, b.L), 7, dtype=torch.int32, device=gpu)
    scores = torch.zeros(N, device=gpu)
    word = torch.zeros(N, dtype=torch.int32, device=gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        b.seed.fill_(11)
        g = o.Graph().capture(lambda: o.token_step(b.logits, V, b.i, b.seed, seqs, scores, word, EOS, PAD, tau=1.0, top_k=40, top_p=1.0))
        g.launch()
        first = seqs[:, b.i].cpu().numpy()
        b.seed.fill_(12)
        g.launch()
        second = seqs[:, b.i].cpu().numpy()
        b.seed.fill_(11)
        g.launch()
        third = seqs[:, b.i].cpu().numpy()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert np.array_equal(first, a1["seqs"][:, b.i]) and np.array_equal(second, c["seqs"][:, b.i]) and np.array_equal(third, first)


# ====================================================================================================== 4. the loop
def _toy_model(seed=5):
    from music_style_transfer.VarAutoEncoder import main, model
    from music_style_transfer.VarAutoEncoder.data import ToyData
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    m = model.Model(main.create_toy_model_config(ToyData())).initialize(gpu_ctx(0), seed=seed)
    batch = next(iter(ToyData(batch_size=6)))  # six sequences: two workgroups of the draw
    return m, batch


def test_the_captured_loop_on_a_toy_token_model(gpu):
    """TokenSampling(keep_logits=True) on a toy token model (the ToyData shape, V = 10), settings (1, 0, 1), (0.7, 5, 1) and
    (1.3, 0, a top_p fitted to the first position's row of sequence 0): every position's token lies in the reference's kept set
    computed from that position's kept logits; PAD follows EOS; scores are the summed -log softmax(logits)[token]; feeding the drawn
    tokens through DecodePlan.step reproduces the kept logits' distributions; decoding twice with one seed gives identical sequences,
    the second run from replayed graphs only.
    Where the fitted top_p is closer than 2 delta to a cumulative mass of some OTHER row (it is fitted to one), an fp32 mass may
    fall on either side of it: the token must then lie in the reference's set for top_p + 2 delta, which contains both."""
    from musicstyletransfer_amd import decode
    m, batch = _toy_model()
    adt = m.store.act_dtype
    tokens, seq_lens, classes = batch.data
    N, L, V = 6, 10, 10
    row0 = m.decoder.initial_rows(tokens, seq_lens, classes)
    ts = decode.TokenSampling(m.store, N, L, keep_logits=True)
    assert m.token_sampling_plan(N, L) is m.token_sampling_plan(N, L)
    ts.run(row0, seed=1)
    first_row = ts.logits[0, 1].cpu().to(adt)             # position 1 depends on row 0 only, whatever is drawn
    fitted = T.fit_top_p(first_row, 1.3, 0, 0.5)[0]
    d = T.delta(V)
    for tau, top_k, top_p in ((1.0, 0, 1.0), (0.7, 5, 1.0), (1.3, 0, fitted)):
        seqs, scores = ts.run(row0, tau=tau, top_k=top_k, top_p=top_p, seed=42)
        n_graphs = len(ts._graphs)
        logits = ts.logits.cpu()
        n = seqs.shape[1]
        assert seqs.shape[0] == N and 2 <= n <= L and ts.positions == n - 1 and (seqs[:, 0] == SOS).all()
        want = np.zeros(N)
        for b in range(N):
            done = False
            for i in range(1, n):
                row = logits[b, i].to(adt)
                assert torch.equal(row.float(), logits[b, i]), "kept logits are the stored 16-bit values"
                if done:
                    assert seqs[b, i] == PAD
                    continue
                kept, _, p = T.token_filter_ref(row, tau, top_k, top_p)
                if top_p < 1.0 and T.margin(row, tau, top_k, top_p) < 2.0:
                    assert (b, i) != (0, 1)
                    kept, _, _ = T.token_filter_ref(row, tau, top_k, min(1.0, top_p + 2 * d))
                assert kept[seqs[b, i]], ((tau, top_k, top_p), b, i, int(seqs[b, i]))
                want[b] += -np.log(p[seqs[b, i]])
                done = seqs[b, i] in (EOS, PAD)
        np.testing.assert_allclose(scores, want, rtol=1e-4, atol=1e-5)
        # teacher-forced: the same tokens through the plain decode step give the same distributions
        plan = decode.DecodePlan(m.store, N, L)
        plan.start(row0)
        for i in range(1, n):
            probs = plan.step(seqs[:, i - 1]).float().cpu().double().numpy()
            ref = torch.softmax(logits[:, i].double(), -1).numpy()
            np.testing.assert_allclose(probs, ref, rtol=1e-4, atol=1e-7)
        again, scores2 = ts.run(row0, tau=tau, top_k=top_k, top_p=top_p, seed=42)
        assert np.array_equal(again, seqs) and np.array_equal(scores2.view(np.uint32), scores.view(np.uint32))
        assert len(ts._graphs) == n_graphs and n_graphs >= n - 1   # nothing captured by the second run
        other, _ = ts.run(row0, tau=tau, top_k=top_k, top_p=top_p, seed=43)
        assert len(ts._graphs) == n_graphs
    assert all(k[0] >= 1 for k in ts._graphs)


# ====================================================================================================== 5. defaults unchanged
def test_defaults_are_the_ancestral_path_and_the_refusals_raise(gpu, monkeypatch):
    from music_style_transfer.VarAutoEncoder import sampler as S
    from musicstyletransfer_amd import decode, generate as G
    monkeypatch.delenv("MST_SAMPLE_DEVICE", raising=False)
    m, batch = _toy_model()
    smp = S.Sampling(seed=1)
    smp.update_parameters(m)
    seqs = smp.sample(batch)
    assert type(smp._dev) is decode.AncestralSampling and seqs.shape[0] == 6
    gen = G.LatentGenerator(m, seed=3)
    out = gen.prior(4, [0, 1, 2, 0], 10)
    assert type(gen.last_sampler) is decode.AncestralSampling and out.sequences.shape == (4, 10)
    for kw in (dict(temperature=0.8), dict(top_k=3), dict(top_p=0.9)):
        smp = S.Sampling(seed=1, **kw)
        smp.update_parameters(m)
        seqs = smp.sample(batch)
        assert type(smp._dev) is decode.TokenSampling and seqs.shape[0] == 6 and (seqs[:, 0] == SOS).all()
        assert np.isfinite(smp.scores).all() and ((seqs >= 0) & (seqs < 10)).all()
    for kw in (dict(sample_temperature=0.8), dict(top_k=3), dict(top_p=0.9)):
        gen = G.LatentGenerator(m, seed=3, **kw)
        out = gen.prior(4, [0, 1, 2, 0], 10)
        assert type(gen.last_sampler) is decode.TokenSampling and out.sequences.shape == (4, 10)
        assert (out.sequences[:, 0] == SOS).all() and np.isfinite(out.scores).all()
    for decoder in ("beam", "greedy"):
        for kw in (dict(top_k=3), dict(top_p=0.5)):
            with pytest.raises(ValueError):
                G.LatentGenerator(m, decoder=decoder, **kw)
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(sample_temperature=0.0)):
        with pytest.raises(ValueError):
            G.LatentGenerator(m, **kw)
    with pytest.raises(ValueError):
        S.Sampling(top_p=0.0)
    # piano-roll models: top_k / top_p raise, sample_temperature is frame_temperature
    from music_style_transfer.VarAutoEncoder import model
    from music_style_transfer.VarAutoEncoder.data import Batch
    from music_style_transfer.VarAutoEncoder.transformer import TransformerConfig
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    P = 48
    pcfg = model.ModelConfig(model.EncoderConfig(TransformerConfig(64, 0.2, 1, 2, P), 16, 2, P),
                             model.DecoderConfig(TransformerConfig(32, 0.2, 1, 2, P), 16, 2, P), kind="pianoroll")
    pm = model.Model(pcfg).initialize(gpu_ctx(0), seed=3)
    x = (np.random.default_rng(0).random((4, 6, P)) < 0.1).astype(np.uint8)
    pbatch = Batch([x, np.full(4, 6, np.int64), np.array([0, 1, 0, 1])], [])
    for kw in (dict(top_k=3), dict(top_p=0.5)):
        with pytest.raises(ValueError):
            G.LatentGenerator(pm, **kw)
        ps = S.Sampling(frames_on_device=True, **kw)
        ps.update_parameters(pm)
        with pytest.raises(ValueError):
            ps.sample(pbatch)
    assert G.LatentGenerator(pm, sample_temperature=0.7).frame_temperature == 0.7
    assert G.LatentGenerator(pm, frame_temperature=0.6).frame_temperature == 0.6
    with pytest.raises(ValueError):
        decode.TokenSampling(pm.store, 4, 8)
