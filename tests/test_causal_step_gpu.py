"""The decoder's opt-in causal mode (VAEConfig.d_causal) through the whole training step on a real GPU, against the oracle with
its decoder attention replaced by the causal restatement (tests/test_causal_cpu.py::causal_attention), and the inference side:
the causal model's teacher-forced forward is what the incremental decoder computes with attention="key", which the samplers
then use by default.

Full-length batches throughout: the encoder keeps the reference's query-axis softmax, whose padded keys put a step in the
mask-flip regime (vae_oracle.FLIP_PRONE); these comparisons assert that regime is not entered."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CFG1 = (128, 128, 2, 64, 256, 2, 8, 128, 1, 8)  # configs[1] / configs[4] widths (scripts/train-vae.sh)


@pytest.fixture
def causal(monkeypatch):
    """the engine's decoder causal (every VAEConfig built while the test runs), the oracle's decoder attention restated"""
    import test_causal_cpu as TC
    from musicstyletransfer_amd import engine as E
    from oracle import vae_oracle as O

    class CausalVAEConfig(E.VAEConfig):
        def __init__(self, *a, **kw):
            kw.setdefault("d_causal", True)
            super().__init__(*a, **kw)

    monkeypatch.setattr(E, "VAEConfig", CausalVAEConfig)
    monkeypatch.setattr(O, "attention", TC.dispatch)
    O.FLIP_PRONE.clear()
    return O


def _step(gpu, O, *a, **kw):
    from test_step_gpu import _compare_step
    plan, store, ot = _compare_step(gpu, *a, ragged=False, **kw)
    assert plan.cfg.d_causal and store.cfg.d_causal
    assert not any(O.FLIP_PRONE.values()), O.FLIP_PRONE
    assert not any(k.startswith("decoder.") for k in O.FLIP_PRONE)  # (the restatement ran for the decoder)
    return plan


def test_toy_token_step(gpu, causal):
    """the reference's --toy configuration and ToyData batch (main.py:14-38, data.py:62-70)"""
    _step(gpu, causal, "token", (10, 10, 3, 16, 32, 1, 2, 32, 1, 2), B=3, T=5, seed=7, steps=2, batch=causal.toy_batch())


def test_small_pianoroll_step(gpu, causal):
    _step(gpu, causal, "pianoroll", (40, 40, 2, 16, 64, 2, 2, 32, 1, 2), B=8, T=45, seed=12, steps=2)


def test_config1_full_size_step_with_riders(gpu, causal):
    """configs[1]'s shape in fp16. In bf16 the probabilities' bulk check measured 2.2e-3 mean error against its 2e-3 bound (every
    other quantity in bounds): a decoder that cannot see its targets predicts in the sigmoid's sensitive range, where bf16
    activation rounding shows; the attention kernels themselves are checked in both types in test_attention_causal_gpu.py, and
    bench.py's bf16 configs[1] step runs causal in test_thirty_steps_train_and_identical_runs_agree_bit_for_bit."""
    plan = _step(gpu, causal, "pianoroll", CFG1, B=64, T=256, seed=1234, steps=1, lr=3e-4, dtype=torch.float16)
    assert plan.forms.riders  # decoder layer 0's projection came from the forward tail's riders


def test_config4_shape_fp16_step(gpu, causal):
    _step(gpu, causal, "pianoroll", CFG1, B=8, T=1024, seed=1024, steps=1, lr=3e-4, dtype=torch.float16, max_err=0.2)


def _token_model(gpu, causal, seed=3):
    from oracle import vae_oracle as O
    from musicstyletransfer_amd.VarAutoEncoder import model
    from musicstyletransfer_amd.VarAutoEncoder.transformer import TransformerConfig
    V, Z = 40, 16

    def t(D, L, H):
        return TransformerConfig(model_size=D, dropout=0.0, num_layers=L, vocab_size=V, num_heads=H)
    cfg = model.ModelConfig(encoder_config=model.EncoderConfig(transformer_config=t(64, 1, 2), latent_dim=Z, num_classes=2, input_dim=V),
                            decoder_config=model.DecoderConfig(transformer_config=t(64, 2, 4), latent_dim=Z, num_classes=2, output_dim=V,
                                                               causal=causal))
    rng = np.random.default_rng(seed)
    params = O.init_params(O.OracleConfig("token", V, V, 2, Z, 64, 1, 2, 64, 2, 4), rng)
    m = model.Model(cfg).initialize(gpu, params_np=params)
    B, T = 5, 9
    x = rng.integers(3, V, size=(B, T))
    x[:, 0] = 1
    return m, x, np.full(B, T), rng.integers(0, 2, size=B)


def test_teacher_forced_forward_equals_incremental_key_decoding(gpu):
    """the test the non-causal decoder fails: Model(...)'s teacher-forced probabilities at positions 1..n are what the KV-cache
    decoder with the softmax over the keys gives when fed the same tokens"""
    m, x, lens, classes = _token_model(gpu, True)
    B, T = x.shape
    probs, mu, sigma = m(x, lens, classes, eps=np.zeros((B, m.engine_config.latent_dim), np.float32))
    tf = probs.float().cpu().numpy()
    row0 = m.decoder.initial_rows(x, lens, classes)  # z = the means, as with eps = 0
    plan = m.decode_plan(B, T + 1)
    assert plan.mode == plan.MODES["key"]
    plan.start(row0)
    inc = np.stack([plan.step(x[:, t]).float().cpu().numpy() for t in range(T)], 1)
    err = np.abs(tf - inc)
    assert err.mean() <= 3e-3 and err.max() <= 6e-2, (err.mean(), err.max())


def test_causal_samplers_default_to_key_attention(gpu):
    from musicstyletransfer_amd.VarAutoEncoder.sampler import BeamSearchSampler, Sampling
    m, x, lens, classes = _token_model(gpu, True)
    s = Sampling()
    s.update_parameters(m)
    assert s.attention == "key"
    b = BeamSearchSampler(beam_size=2)
    b.update_parameters(m)
    assert b.attention == "key"
    q = Sampling(attention="query")
    q.update_parameters(m)
    with pytest.raises(ValueError):
        q.attention
    with pytest.raises(ValueError):
        m.decode_plan(2, 4, "query")
    with pytest.raises(ValueError):
        m.decoder.get_initial_state(x, lens, classes, t_max=4, attention="query")
    state = m.decoder.get_initial_state(x, lens, classes, t_max=4)
    assert state.plan.mode == state.plan.MODES["key"]
    plain, *_ = _token_model(gpu, False)
    s.update_parameters(plain)
    assert s.attention == "query"


def test_thirty_steps_train_and_identical_runs_agree_bit_for_bit(gpu):
    """bench.py's configs[1] step (dropout 0.2, internal eps) with the causal decoder: 30 steps on one batch stay finite and lower
    the loss; two identical runs agree bit for bit over their first two steps (the span tests/test_step_gpu.py's benchmark-step
    check covers for the default decoder)."""
    from musicstyletransfer_amd import engine as E
    dims = dict(kind="pianoroll", in_dim=128, out_dim=128, num_classes=2, latent_dim=64, e_model=256, e_layers=2, e_heads=8,
                d_model=128, d_layers=1, d_heads=8)
    B, T = 64, 256
    rng = np.random.default_rng(77)
    roll = (rng.random((B, T + 1, 128)) < 0.04).astype(np.uint8)
    x = roll[:, :T].copy()
    x[:, 0, :] = 0
    x[:, 0, 0] = 1
    classes = rng.integers(0, 2, size=B).astype(np.int32)
    runs = []
    for n_steps in (30, 2):
        store = E.ParamStore(E.VAEConfig(e_dropout=0.2, d_dropout=0.2, d_causal=True, **dims), gpu, torch.bfloat16, seed=1234)
        plan = E.StepPlan(store, B, T, lr=1e-3, clip_gradient=1.0, kl_weight=1.0, global_batch=B, internal_eps=True, seed=1000)
        plan.bind_inputs(plan.pack_batch(x, np.full(B, T, np.int32), classes, roll[:, 1:].copy()).to(gpu))
        losses, ws = [], []
        for _ in range(n_steps):
            plan.step_kernels(True)
            losses.append(float(plan.total.mean().item()))
            if len(ws) < 2:
                ws.append((store.to_numpy("g"), store.w.cpu().numpy().copy()))
        torch.cuda.synchronize()
        runs.append((losses, ws, store.read_metrics(reset=False)["skipped_steps"]))
        del plan, store
    losses = runs[0][0]
    assert np.all(np.isfinite(losses)), losses
    assert np.mean(losses[-5:]) < 0.9 * np.mean(losses[:3]), losses
    assert runs[1][0] == losses[:2], (runs[0][2], runs[1][2])
    for i, ((ga, wa), (gb, wb)) in enumerate(zip(runs[0][1], runs[1][1])):
        differ = [n for n in ga if not np.array_equal(ga[n], gb[n])]
        assert not differ and np.array_equal(wa, wb), f"step {i + 1}: {differ}"
