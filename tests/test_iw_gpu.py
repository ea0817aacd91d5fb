"""The importance-weighted bound on the GPU: mst_iw_fold / mst_iw_finish against the fp64 reference (tests/iw_refs.py), the engine's
draw pass against the full inference forward, engine.IWBound against the reference folded over the draws it recorded and against the
CPU oracle, and the trainer / command-line surface.

Kernel-level bounds (iw_refs.compare): m, sum_lw, log_px, elbo within 1e-10 * (1 + sum |terms|); s, s2, ess within 1e-9 relative.
Engine level against the oracle: the batch mean of log_px within 1e-3 of the batch-mean reconstruction term in nats (the recon tolerance
of test_step_gpu._compare_step) plus 2e-3 of the batch-mean KL (its ELBO tolerance)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iw_refs as R  # noqa: E402
from test_iw_cpu import ENGINE_CASES  # noqa: E402
from test_step_gpu import _setup  # noqa: E402

pytestmark = pytest.mark.gpu
MIDI = os.path.join(ROOT, "tests", "golden", "midi")
EPS_SITE = 0x7FFF0000  # include/mst_hip.h: mst_step_begin's eps site
DTYPES = [torch.bfloat16, torch.float16]
U64 = 0xFFFFFFFFFFFFFFFF


# ====================================================================================================== 1. the two launches
def _padded(gpu, a, pad):
    """host [B, Z] -> the [B, Z] view of a device [B, Z + pad] tensor whose pad columns hold NaN (never read)"""
    B, Z = a.shape
    t = torch.full((B, Z + pad), float("nan"), dtype=torch.float32, device=gpu)
    t[:, :Z] = torch.from_numpy(np.ascontiguousarray(a))
    return t[:, :Z]


def _fold_on_device(gpu, case, acc=None):
    from musicstyletransfer_amd import ops as o
    K, B = case["recon"].shape
    f64 = dict(dtype=torch.float64, device=gpu)
    state, out = torch.zeros(B, 6, **f64), torch.zeros(B, 4, **f64)
    acc = torch.zeros(6, **f64) if acc is None else acc
    for k in range(K):
        o.iw_fold(_padded(gpu, case["eps"][k], 3), _padded(gpu, case["sigma"][k], 8), _padded(gpu, case["z"][k], 0),
                  torch.from_numpy(case["recon"][k]).to(gpu), case["recon_scale"], state)
    o.iw_finish(state, out, acc)
    torch.cuda.synchronize()
    return state.cpu().numpy(), out.cpu().numpy(), acc


@pytest.mark.parametrize("draws", R.KERNEL_DRAWS)
@pytest.mark.parametrize("B,Z", R.KERNEL_SHAPES)
def test_fold_and_finish_against_the_fp64_reference(gpu, B, Z, draws):
    case = R.kernel_case(B, Z, draws)
    want_state, mag = R.fold_case(case)
    before = np.array([1.5, -2.5, 3.0, 4.0, 5.0, 6.0])
    want_out, want_acc = R.finish(want_state, acc=before)
    acc = torch.from_numpy(before.copy()).to(gpu)
    state, out, acc = _fold_on_device(gpu, case, acc)
    bad = R.compare(state, out, want_state, want_out, mag)
    assert not bad, "\n".join(bad)
    # a special sample ends invalid with only n_bad touched by its bad draw; every other row is a row of the reference (above)
    for b, what in R.special_rows(B).items():
        if what in ("sigma0", "nan_eps", "inf_recon"):
            assert state[b, R.N_BAD] == 1 and state[b, R.N] == draws - 1 and np.isnan(out[b, :3]).all() and out[b, 3] == draws - 1
    # acc is ADDED to: the counts exactly, the sums to the bound of their terms
    got = acc.cpu().numpy()
    valid = ~np.isnan(want_out[:, 0])
    assert got[3:].tolist() == want_acc[3:].tolist()
    assert np.abs(got[:2] - want_acc[:2]).max() <= R.ABS_TOL * (1.0 + mag[valid].sum() + np.abs(before).sum())
    assert abs(got[2] - want_acc[2]) <= R.REL_TOL * (abs(want_acc[2]) + abs(before[2]))
    # the same launches on the same inputs: the same bits; a second finish adds the same sums again
    state2, out2, acc2 = _fold_on_device(gpu, case, acc)
    assert state2.tobytes() == state.tobytes() and out2.tobytes() == out.tobytes()
    twice = acc2.cpu().numpy()
    assert twice[3:].tolist() == (2 * want_acc[3:] - before[3:]).tolist()
    np.testing.assert_allclose(twice[:3] - got[:3], got[:3] - before[:3], rtol=1e-9, atol=1e-9 * (1 + np.abs(got[:3]).max()))


def test_bad_arguments_return_a_status(gpu):
    from musicstyletransfer_amd import _lib, ops as o
    f = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=gpu)
    state, out, acc = f(3, 6, dt=torch.float64), f(3, 4, dt=torch.float64), f(6, dt=torch.float64)
    with pytest.raises(_lib.MstError, match="recon_scale"):
        o.iw_fold(f(3, 8), f(3, 8), f(3, 8), f(3), 0.0, state)
    with pytest.raises(_lib.MstError, match="16-byte aligned"):
        o.iw_finish(f(4, 6, dt=torch.float64).view(-1)[1:19].view(3, 6), out, acc)
    with pytest.raises(AssertionError):
        o.iw_fold(f(3, 8), f(3, 8), f(3, 7), f(3), 1.0, state)
    torch.cuda.synchronize()
    assert not state.any().item() and not acc.any().item()


# ====================================================================================================== 2. the engine
CASES = dict(ENGINE_CASES)
CASES["roll-riders"] = ("pianoroll", (64, 64, 2, 16, 128, 2, 4, 128, 1, 4), 4, 128, 304)  # T % 128 == 0, De = Dd = 128: the forward tail's riders
_ctx_cache = {}


class Ctx:
    """one model and batch of a case, on the device in one 16-bit type, with a plan that draws its own eps"""

    def __init__(self, gpu, name, dtype, **hyper):
        kind, dims, B, T, seed = CASES[name]
        self.kind, self.dims, self.B, self.T = kind, dims, B, T
        self.O, self.E, self.ocfg, self.ecfg, self.params, self.batch, self.eps = _setup(kind, dims, B, T, seed)
        self.store = self.E.ParamStore(self.ecfg, gpu, dtype, params_np=self.params)
        self.plan = self.new_plan(internal_eps=True, **hyper)
        self.cells = T * (dims[1] if kind == "pianoroll" else 1)

    def new_plan(self, B=None, rows=slice(None), **hyper):
        plan = self.E.StepPlan(self.store, B or self.B, self.T, **hyper)
        b = self.batch
        plan.load_batch(b["x"][rows], b["seq_lens"][rows], b["classes"][rows], b["labels"][rows])
        return plan

    def run(self, K, plan=None, keep_draws=False, rng=None):
        """IWBound of `plan` (default: the case's) from K draws, the inference RNG stream set to `rng` first (None: as it is);
        -> (runner, host copies of state / out / acc, the recorded draws as host arrays or None)"""
        st = self.store
        if rng is not None:
            st.rng_state_inference().copy_(rng)
        iw = self.E.IWBound(plan or self.plan)
        iw.run(K, keep_draws=keep_draws, reset_acc=True)
        torch.cuda.synchronize()
        draws = {k: v.cpu().numpy() for k, v in iw.draws.items()} if keep_draws else None
        return iw, iw.state.cpu().numpy(), iw.out.cpu().numpy(), iw.acc.cpu().numpy(), draws


def _ctx(gpu, name, dtype):
    key = (name, dtype)
    if key not in _ctx_cache:
        c = _ctx_cache[key] = Ctx(gpu, name, dtype)
        c.rng0 = c.store.rng_state_inference().clone()
        c.rec = c.run(4, keep_draws=True, rng=c.rng0)  # the K = 4 run with recorded draws that several tests below share
    return _ctx_cache[key]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_draw_pass_is_the_decoder_half_of_the_full_forward(gpu, name, dtype):
    """given eps E the draw pass leaves what forward(inference=True) with eps E leaves — also for an E the encoder never saw with the
    rows it reuses, i.e. after a full forward at ANOTHER eps"""
    c = _ctx(gpu, name, dtype)
    B, T, Z = c.B, c.T, c.dims[3]
    plan = c.new_plan(internal_eps=False)
    rng = np.random.default_rng(11)
    E1, E2 = (rng.standard_normal((B, Z)).astype(np.float32) for _ in range(2))
    names = ("mu", "sigma", "z", "kl")
    row0 = lambda: plan.x0_d.view(B, T + 1, -1)[:, 0, :]

    def full(eps):
        plan.eps.copy_(torch.from_numpy(eps))
        plan.forward(inference=True)
        plan.losses(with_grad=False, combine=False, plain=True)
        torch.cuda.synchronize()
        return {k: _bits(getattr(plan, k)) for k in names}, _bits(row0()), plan.recon.cpu().numpy().copy()

    want2 = full(E2)
    want1 = full(E1)  # (the encoder output and decoder rows 1..T the draw passes below reuse are this forward's)
    one_wg = c.kind == "pianoroll" and plan.forms.fuse_bce and T == 64  # a 64-row tile of the fused loss launch is one sample's rows
    for eps, (lat, r0, recon) in ((E1, want1), (E2, want2), (E1, want1)):
        for k in names:
            getattr(plan, k).fill_(float("nan"))
        row0().zero_()
        plan.recon.fill_(123.0)
        plan.eps.copy_(torch.from_numpy(eps))
        plan.forward(inference=True, start="latent")
        plan.losses(with_grad=False, combine=False, plain=True)
        torch.cuda.synchronize()
        for k in names:
            assert _bits(getattr(plan, k)) == lat[k], f"{k} of the draw pass differs from the full forward's"
        assert _bits(row0()) == r0, "decoder row 0"
        got = plan.recon.cpu().numpy()
        assert np.isfinite(got).all() and (np.abs(got - recon) <= 1e-6 * np.abs(recon)).all(), (got, recon)
        if one_wg:
            assert got.tobytes() == recon.tobytes()
    print(f"\n{name} {dtype}: forms riders={plan.forms.riders} tails={plan.forms.tails} fuse_bce={plan.forms.fuse_bce} one_wg={one_wg}")
    with pytest.raises(ValueError):
        plan.forward(start="latent")
    with pytest.raises(ValueError):
        plan.forward(inference=True, start="latent", upto="latent")
    with pytest.raises(RuntimeError, match="preceding full"):
        c.E.StepPlan(c.store, B, T).forward(inference=True, start="latent")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_the_runner_is_the_reference_folded_over_its_recorded_draws(gpu, name, dtype):
    from musicstyletransfer_amd import ops as o
    c = _ctx(gpu, name, dtype)
    iw, state, out, acc, d = c.rec
    K, B, Z = 4, c.B, c.dims[3]
    assert iw.recon_scale == c.cells
    st, mag = np.zeros((B, 6)), np.zeros(B)
    for k in range(K):
        lw, m = R.log_weight(d["eps"][k], d["sigma"][k], d["z"][k], d["recon"][k], iw.recon_scale)
        st, mag = R.fold_lw(st, lw), mag + m
    want_out, want_acc = R.finish(st)
    bad = R.compare(state, out, st, want_out, mag)
    assert not bad, "\n".join(bad)
    assert acc[3:].tolist() == [K * B, B, 0] and np.abs(acc[:2] - want_acc[:2]).max() <= R.ABS_TOL * (1 + mag.sum())
    res = iw.results()
    assert res["valid"].all() and np.array_equal(res["log_px"], out[:, 0]) and np.array_equal(res["n"], np.full(B, K))
    # draw k's eps is mst_randn at the seed the draw's bookkeeping launch left, the eps site, element index (sample_offset + b) * Z + d
    seeds = [int(s) & U64 for s in d["seed"]]
    assert len(set(seeds)) == K, "every draw has a seed of its own"
    buf = torch.zeros(B * Z, dtype=torch.float32, device=gpu)
    for k in range(K):
        o.randn(buf, seed=seeds[k], site=EPS_SITE)
        assert _bits(buf) == d["eps"][k].tobytes(), f"eps of draw {k}"
    # sigma does not depend on the draw; z = mu + eps sigma does
    assert all(d["sigma"][k].tobytes() == d["sigma"][0].tobytes() for k in range(K)) and d["z"][1].tobytes() != d["z"][0].tobytes()
    # a plan with sample_offset = 2 draws rows 2..3 of what the 4-sample plan draws (from the same stream of seeds)
    half = c.new_plan(B=2, rows=slice(2, 4), internal_eps=True, sample_offset=2)
    _, _, out2, _, d2 = c.run(K, plan=half, keep_draws=True, rng=c.rng0)
    assert d2["seed"].tolist() == d["seed"].tolist() and d2["eps"].tobytes() == np.ascontiguousarray(d["eps"][:, 2:4]).tobytes()
    assert np.abs(out2[:, 0] - out[2:4, 0]).max() <= 1e-5 * np.abs(out[2:4, 0]).max()  # (the pieces themselves: the same bound, atomics aside)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_the_bound_against_the_oracle(gpu, name, dtype):
    """oracle.model_forward at the recorded eps gives recon, mu and sigma; iw_refs folds them into a reference bound"""
    c = _ctx(gpu, name, dtype)
    _, _, out, _, d = c.rec
    O, P = c.O, c.O.to_torch_params(c.params, requires_grad=False)
    st, nats, kls = np.zeros((c.B, 6)), [], []
    for k in range(4):
        e = torch.from_numpy(d["eps"][k])
        with torch.no_grad():
            _, recon, kl, _, means, stds = O.step_losses(P, c.ocfg, c.batch, e)
        st = R.fold(st, e.numpy(), stds.numpy(), (means + e * stds).numpy(), recon.numpy(), float(c.cells))
        nats.append(c.cells * recon.numpy().astype(np.float64))
        kls.append(kl.numpy().astype(np.float64))
    want, _ = R.finish(st)
    assert np.isfinite(want).all(), "the oracle leaves no sample invalid"
    tol = 1e-3 * np.mean(nats) + 2e-3 * np.mean(kls)
    err = abs(out[:, 0].mean() - want[:, 0].mean())
    print(f"\n{name} {dtype}: mean log_px {out[:, 0].mean():.6f} oracle {want[:, 0].mean():.6f} |diff| {err:.3g} bound {tol:.3g} "
          f"(recon nats {np.mean(nats):.4f}, KL {np.mean(kls):.4f}); elbo {out[:, 1].mean():.6f} vs {want[:, 1].mean():.6f}; "
          f"ess {out[:, 2].mean():.4f} vs {want[:, 2].mean():.4f}")
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_jensen_gap_ess_range_and_one_draw(gpu, name, dtype):
    c = _ctx(gpu, name, dtype)
    _, state, out, acc, _ = c.rec
    assert (out[:, 0] - out[:, 1] >= -1e-10 * (1 + np.abs(out[:, 1]))).all(), "iw_gap >= 0 per piece"
    assert (out[:, 2] >= 1 - 1e-9).all() and (out[:, 2] <= 4 + 1e-9).all(), "1 <= ess <= K"
    s = c.E.iw_scores(acc, c.cells)
    assert s["iw_gap"] >= -1e-10 * abs(s["iw_nll"]) and 1 - 1e-9 <= s["iw_ess"] <= 4 + 1e-9 and s["iw_invalid"] == 0
    assert s["iw_bits_per_cell"] > 0
    _, state1, out1, acc1, _ = c.run(1)
    assert out1[:, 0].tobytes() == out1[:, 1].tobytes() == state1[:, R.M].tobytes() and (out1[:, 2] == 1).all() and (out1[:, 3] == 1).all()
    assert acc1[3:].tolist() == [c.B, c.B, 0]


@pytest.mark.parametrize("name", ["roll-d128", "roll-d64"])
def test_label_smoothing_and_downscaling_do_not_reach_the_bound(gpu, name):
    """a plan trained with label smoothing and --negative-label-downscaling reports the bound of the plain likelihood"""
    c = Ctx(gpu, name, torch.bfloat16)
    trained = c.new_plan(internal_eps=True, label_smoothing=0.1, negative_label_downscaling=True, lr=1e-3)
    trained.step_kernels(True)  # (one training step with them: the weights both plans share move)
    plain = c.new_plan(internal_eps=True)
    rng0 = c.store.rng_state_inference().clone()
    _, _, out_t, _, _ = c.run(4, plan=trained, rng=rng0)
    _, _, out_p, _, _ = c.run(4, plan=plain, rng=rng0)
    scale = np.abs(out_p[:, 1])  # (the ELBO in nats: the reconstruction term dominates it)
    assert np.isfinite(out_t).all() and (np.abs(out_t[:, :2] - out_p[:, :2]) <= 1e-6 * scale[:, None]).all(), (out_t, out_p)
    assert (np.abs(out_t[:, 2] - out_p[:, 2]) <= 1e-3 * out_p[:, 2]).all()
    # ... and the training loss of that plan is another number: the override is what makes them agree
    recon = {}
    for plain_loss in (False, True):
        c.store.rng_state_inference().copy_(rng0)  # (the same eps both times)
        trained.forward(inference=True)
        trained.losses(with_grad=False, combine=False, plain=plain_loss)
        recon[plain_loss] = trained.recon.cpu().numpy().copy()
    assert (np.abs(recon[True] - recon[False]) > 1e-3 * np.abs(recon[False])).all()


@pytest.mark.parametrize("name", ["roll-d128", "token", "roll-riders"])
def test_one_graph_for_eight_draws_and_no_encoder_launch_in_it(gpu, name):
    from musicstyletransfer_amd import ops as o
    c = Ctx(gpu, name, torch.bfloat16)
    iw = c.E.IWBound(c.plan)
    iw.run(8)
    torch.cuda.synchronize()
    assert iw.captures == 1 and (iw.out[:, 3] == 8).all().item()
    first = iw.out.cpu().numpy().copy()
    iw.run(8)
    iw.run(3)
    torch.cuda.synchronize()
    assert iw.captures == 1, "later runs replay the graph captured first"
    assert (iw.out[:, 3] == 3).all().item() and np.isfinite(first).all()
    nodes, kernels = iw.graph_nodes()
    plan = c.plan
    with torch.cuda.stream(torch.cuda.Stream()):
        full = o.Graph().capture(lambda: (plan.forward(inference=True), plan.losses(with_grad=False, combine=False, plain=True)))
        enc = o.Graph().capture(lambda: plan.forward(inference=True, upto="latent"))
    torch.cuda.synchronize()
    # the draw pass = the full pass without the launches up to the latent block, plus its own bookkeeping launch, the latent launch
    # and the fold; the token ends' decoder embedding (rows 1..T, which do not depend on z) is not re-issued
    want = full.kernel_nodes - enc.kernel_nodes + 3 - (1 if c.kind == "token" else 0)
    print(f"\n{name}: draw pass {kernels} kernel launches ({nodes} nodes), full pass {full.kernel_nodes}, up to the latent block {enc.kernel_nodes}")
    assert kernels == want and kernels < full.kernel_nodes + 1


# ====================================================================================================== 3. trainer and command line
IW_KEYS = ("iw_nll", "iw_elbo_nll", "iw_gap", "iw_ess", "iw_bits_per_cell", "iw_invalid")


def _small_trainer(params, dims, B, iw_samples):
    """a Trainer on a small piano-roll model, from the weights of _setup (tests/test_ema_gpu.py builds its trainers the same way)"""
    from music_style_transfer.VarAutoEncoder import model, trainer
    from music_style_transfer.VarAutoEncoder.transformer import TransformerConfig
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    P, _, C, Z, De, Le, He, Dd, Ld, Hd = dims
    mc = model.ModelConfig(model.EncoderConfig(TransformerConfig(De, 0.0, Le, He, P), Z, C, P),
                           model.DecoderConfig(TransformerConfig(Dd, 0.0, Ld, Hd, P), Z, C, P), kind="pianoroll")
    cfg = trainer.TrainConfig(batch_size=B, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                              optimizer=trainer.OptimizerConfig(learning_rate=1e-3, optimizer="adam", optimizer_params="clip_gradient:1.0"),
                              kl_loss=1.0, label_smoothing=0.1, negative_label_downscaling=True, verbose=False, iw_samples=iw_samples)
    t = trainer.Trainer(config=cfg, context=gpu_ctx(0), model=model.Model(mc), sampler=None)
    with torch.cuda.stream(t.stream):
        t.model.store.load_numpy(params)
    t.stream.synchronize()
    return t


def test_six_steps_with_the_bound_in_the_middle_end_with_the_same_weights(gpu, tmp_path, capsys):
    """three steps, a checkpoint whose validation carries the bound from three draws, three more steps: the weights and moments of the
    same six steps and checkpoint without it, bit for bit. Asserted, as everywhere between two trainers, on the fixed-order form of the
    LayerNorm backward (StepPlan.LN_PARTIALS_MIN = 0: the default form at this size adds d gamma / d beta with fp32 atomics and is not
    bit-identical to itself)."""
    import types
    from musicstyletransfer_amd import engine as E
    dims, B, T = (128, 128, 3, 32, 64, 1, 4, 64, 2, 4), 4, 33  # the small model and shape of tests/test_ema_gpu.py's trainers
    _, _, _, _, params, b, _ = _setup("pianoroll", dims, B, T, 13, ragged=True)
    batch = types.SimpleNamespace(data=[b["x"], b["seq_lens"], b["classes"]], label=[b["labels"]])
    was = E.StepPlan.LN_PARTIALS_MIN
    E.StepPlan.LN_PARTIALS_MIN = 0
    try:
        runs = {}
        for K in (0, 3, 0):
            t = _small_trainer(params, dims, B, K)
            for _ in range(3):
                t._step(batch)
                t.train_state.n_batches += 1
            capsys.readouterr()
            t._checkpoint(str(tmp_path / f"m{K}{len(runs)}"), [batch])
            line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Checkpoint [")]
            for _ in range(3):
                t._step(batch)
                t.train_state.n_batches += 1
            t.stream.synchronize()
            torch.cuda.synchronize()
            st = t.model.store
            assert int(st.step_state[0].item()) == 6
            snap = tuple(_bits(getattr(st, k)) for k in ("w", "m", "v", "w16"))
            if K == 0 and 0 in runs:  # (the yardstick: without the option the six steps are bit-identical to themselves)
                assert snap == runs[0][0], "two runs without the option differ: the comparison below would show nothing"
            else:
                runs[K] = (snap, t.last_validation, line, t)
    finally:
        E.StepPlan.LN_PARTIALS_MIN = was
    assert runs[3][0] == runs[0][0], "the bound must leave the training trajectory alone"
    v, v0 = runs[3][1], runs[0][1]
    assert set(IW_KEYS) <= set(v) and not set(IW_KEYS) & set(v0)
    assert v["total_loss"] == v0["total_loss"] and v["kl_loss"] == v0["kl_loss"]  # (the usual validation figures are untouched)
    line = runs[3][2]
    assert len(line) == 1 and all(k + "=" in line[0] for k in IW_KEYS), line
    assert not any(k + "=" in runs[0][2][0] for k in IW_KEYS)
    assert np.isfinite([v[k] for k in IW_KEYS]).all() and v["iw_gap"] >= 0 and 1 <= v["iw_ess"] <= 3 and v["iw_invalid"] == 0
    # the figures are those of the runner on the same batch and weights: nats per piece, T * P cells
    t = runs[3][3]
    assert abs(v["iw_bits_per_cell"] - v["iw_nll"] / (T * 128 * np.log(2.0))) <= 1e-12 * v["iw_bits_per_cell"]
    assert t._iw_acc is not None and t._last_plan.__dict__.get("_iw") is not None and t._last_plan._iw.acc is t._iw_acc


def test_the_flag_through_the_entry_point_and_the_scalar_log(gpu, tmp_path, monkeypatch, capsys):
    import json
    from music_style_transfer.VarAutoEncoder import main
    from music_style_transfer.VarAutoEncoder.data import ToyData
    monkeypatch.setenv("MST_LOGDIR", str(tmp_path / "tb"))
    folder = str(tmp_path / "toy")
    t = main.main(["--toy", "--gpu", "--max-steps", "3", "--model-output", folder, "--iw-samples", "3"])
    assert t.config.iw_samples == 3 and t.iw_samples == 3
    capsys.readouterr()
    t._checkpoint(os.path.join(folder, "model"), ToyData())
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Checkpoint [")]
    v = t.last_validation
    assert len(line) == 1 and all(k + "=" in line[0] for k in IW_KEYS) and "total_loss=" in line[0], line
    assert np.isfinite([v[k] for k in IW_KEYS]).all() and v["iw_gap"] >= 0 and 1 <= v["iw_ess"] <= 3 and v["iw_invalid"] == 0
    t._step(next(iter(ToyData())))  # (training goes on: the graphs of the shape are still the trainer's)
    t.stream.synchronize()
    t.summary_writer.flush()
    tags = {json.loads(ln)["tag"] for ln in open(tmp_path / "tb" / "scalars.jsonl")}
    assert set(IW_KEYS) <= tags


def test_generate_mode_likelihood_on_the_golden_midi(gpu, tmp_path, capsys):
    from music_style_transfer.VarAutoEncoder import generate as G, main, utils
    folder = str(tmp_path / "m")
    t = main.main(["--gpu", "--batch-size", "4", "--max-seq-len", "32", "--validation-split", "0.0", "--e-n-layers", "1",
                   "--e-rnn-hidden-dim", "64", "--d-rnn-hidden-dim", "64", "--e-num-heads", "4", "--latent-dim", "16", "--max-steps", "2",
                   "--sampling-frequency", "0", "--data", MIDI, "--model-output", folder, "--out-samples", str(tmp_path / "s")])
    t.stream.synchronize()
    torch.cuda.synchronize()
    utils.save_model(t.model, os.path.join(folder, "params.0"))
    capsys.readouterr()
    before = set(os.listdir(folder))
    lines = G.main(["--model-output", folder, "--checkpoint", "-1", "--data", MIDI, "--batch-size", "4", "--max-seq-len", "32",
                    "--mode", "likelihood", "--iw-samples", "4"])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("melody ")]
    assert len(lines) == 4 and printed == lines and set(os.listdir(folder)) == before  # one line per melody, no files
    for i, ln in enumerate(lines):
        w = ln.split()
        assert w[:2] == ["melody", str(i)] and w[4::2] == ["nll", "elbo_nll", "ess", "bits_per_cell", "valid"] and w[-1] == "1"
        nll, elbo_nll, ess, bits = (float(x) for x in w[5:12:2])
        assert np.isfinite([nll, elbo_nll, ess, bits]).all() and elbo_nll >= nll - 1e-6 * abs(nll) and 1 <= ess <= 4
    with pytest.raises(ValueError, match="iw_samples"):
        G.main(["--model-output", folder, "--data", MIDI, "--batch-size", "4", "--max-seq-len", "32", "--mode", "likelihood", "--iw-samples", "0"])
