"""Latent-space generation on a real GPU: mst_latent_rows against an fp64 restatement, the identity recipe against the existing
path, the noise, spherical interpolation, mst_frame_step, the FrameSampling loop, the restyled melody against the oracle, and the
public interface on the toy model."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # half a unit in the last place, relative to the binade's lower end


def _half_ulp(x, adt):
    """half a unit in the last place of `adt` at the magnitude of x (fp64 array)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14 if adt == torch.float16 else 2.0 ** -126)))
    return 2.0 ** e * ULP[adt]


def _tables(rng, Z, Dd, C, gpu):
    t = dict(Wh=0.3 * rng.standard_normal((Dd, Z)), bh=0.1 * rng.standard_normal(Dd), cls=rng.standard_normal((C, Dd)),
             pos=rng.standard_normal((1, Dd)))
    t = {k: v.astype(np.float32) for k, v in t.items()}
    return t, {k: torch.from_numpy(v).to(gpu) for k, v in t.items()}


def _rows(gpu, dev_t, zsrc, ssrc, a, b, w, ca, cb, cw, Dd, adt, **kw):
    from musicstyletransfer_amd import ops as o
    up = lambda x, d: None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, d))).to(gpu)
    N = len(ca)
    Z = dev_t["Wh"].shape[1]
    z_out = torch.full((N, Z), 7.0, dtype=torch.float32, device=gpu)
    dec = torch.zeros(N, Dd + 8, dtype=adt, device=gpu)
    o.latent_rows(up(zsrc, np.float32), up(ssrc, np.float32), up(a, np.int32), up(b, np.int32), up(w, np.float32), up(ca, np.int32),
                  up(cb, np.int32), up(cw, np.float32), dev_t["Wh"], dev_t["bh"], dev_t["cls"], dev_t["pos"], kw.pop("alpha", 1.0), z_out, dec, **kw)
    torch.cuda.synchronize()
    assert (dec[:, Dd:] == 0).all()  # nothing behind the row
    return z_out.cpu().numpy(), dec[:, :Dd].float().cpu().numpy().astype(np.float64)


def _interp64(za, zb, w, mode):
    """-> (base, sum of |terms|) in fp64; the spherical form as include/mst_hip.h states it"""
    fa, fb = 1.0 - w, w
    if mode == "slerp" and 0.0 < w < 1.0:
        na, nb = np.linalg.norm(za), np.linalg.norm(zb)
        c = za @ zb / (na * nb) if na > 0 and nb > 0 else 2.0
        if abs(c) < 1.0 - 2.0 ** -16:
            om = np.arccos(c)
            fa, fb = np.sin((1 - w) * om) / np.sin(om), np.sin(w * om) / np.sin(om)
    elif mode == "slerp":
        fa, fb = (1.0, 0.0) if w <= 0 else (0.0, 1.0)
    return fa * za + fb * zb, np.abs(fa * za) + np.abs(fb * zb)


@pytest.mark.parametrize("adt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Z,Dd", [(16, 32), (64, 128), (256, 256), (64, 32), (16, 256)])
def test_latent_rows_matches_an_fp64_restatement(gpu, adt, Z, Dd):
    """every mode — identity, lerp, slerp, prior, posterior, class blend — in ONE recipe of N = 37 rows.
    Bounds (derived, not measured): a value formed in fp32 from n_t terms by products and sums carries at most n_t roundings of
    2^-24 relative to the sum of the terms' magnitudes; with the factor 8 for the elementary functions (sin, acos, the division) and
    the two interpolation factors this is |err(z)| <= 8 Z 2^-24 sum|terms| (Z >= 16 terms bound every chain here, the dot product
    of the spherical form included). A row adds the Z-term dot product with Wh, the bias, the two class terms and the position in
    fp32 — the same bound on ITS terms — and one rounding to the activation type: half a unit in the last place at the row's
    magnitude. With tau > 0 the eps the kernel drew is recovered from z_out, so the arithmetic check does not restate the hash."""
    rng = np.random.default_rng(Z * 1000 + Dd)
    M, C, N, alpha, tau = 9, 3, 37, float(np.sqrt(Dd)), 0.75
    host, dev = _tables(rng, Z, Dd, C, gpu)
    zsrc = rng.standard_normal((M, Z)).astype(np.float32)
    ssrc = (0.5 + rng.random((M, Z))).astype(np.float32)
    kinds = ["identity", "lerp", "slerp", "prior", "posterior", "blend"]
    kind = [kinds[n % 6] for n in range(N)]
    a = rng.integers(0, M, N); b = rng.integers(0, M, N); w = rng.random(N).astype(np.float32)
    ca = rng.integers(0, C, N); cb = rng.integers(0, C, N); cw = rng.random(N).astype(np.float32)
    for n, k in enumerate(kind):
        if k in ("identity", "posterior", "blend", "prior"):
            b[n], w[n] = a[n], 0.0
        if k == "prior":
            a[n] = b[n] = -1
        if k != "blend":
            cb[n], cw[n] = ca[n], 0.0
    for mode in ("lerp", "slerp"):
        for use_tau, use_s in ((0.0, False), (tau, True), (tau, False)):
            z, rows = _rows(gpu, dev, zsrc, ssrc if use_s else None, a, b, w, ca, cb, cw, Dd, adt, alpha=alpha, mode=mode, tau=use_tau, seed=11)
            for n in range(N):
                if a[n] < 0:
                    base, mag, scale = np.zeros(Z), np.zeros(Z), np.ones(Z)
                else:
                    base, mag = _interp64(zsrc[a[n]].astype(np.float64), zsrc[b[n]].astype(np.float64), float(w[n]), mode)
                    scale = ((1.0 - float(w[n])) * ssrc[a[n]] + float(w[n]) * ssrc[b[n]]).astype(np.float64) if use_s else np.ones(Z)
                if use_tau > 0:
                    eps = (z[n].astype(np.float64) - base) / (use_tau * scale)  # the eps the kernel drew
                    assert np.isfinite(eps).all() and np.abs(eps).max() < 7.0
                    want_z, mag = base + use_tau * eps * scale, mag + np.abs(use_tau * eps * scale)
                    if a[n] < 0:
                        assert np.abs(eps).max() > 0  # a prior row IS noise
                else:
                    want_z = base
                    assert (np.abs(z[n] - want_z) <= 8 * Z * 2.0 ** -24 * mag + 1e-30).all(), (mode, kind[n], n)
                zz = z[n].astype(np.float64)  # the row is built from the z the kernel stored
                cls = (1.0 - float(cw[n])) * host["cls"][ca[n]].astype(np.float64) + float(cw[n]) * host["cls"][cb[n]].astype(np.float64)
                inner = host["Wh"].astype(np.float64) @ zz + host["bh"] + cls
                want = alpha * inner + host["pos"][0]
                terms = alpha * (np.abs(host["Wh"].astype(np.float64)) @ np.abs(zz) + np.abs(host["bh"]) + np.abs(cls)) + np.abs(host["pos"][0])
                f32 = 8 * Z * 2.0 ** -24 * terms
                bound = f32 + _half_ulp(np.abs(want) + f32, adt)  # (the fp32 value that is rounded may sit that much higher)
                assert (np.abs(rows[n] - want) <= bound).all(), (mode, kind[n], n, np.abs(rows[n] - want).max())


def _pianoroll_model(gpu, dims=(48, 48, 2, 16, 64, 1, 2, 32, 1, 2), causal=False, seed=3):
    from music_style_transfer.VarAutoEncoder import model
    from music_style_transfer.VarAutoEncoder.transformer import TransformerConfig
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    from oracle import vae_oracle as O
    P, _, C, Z, De, Le, He, Dd, Ld, Hd = dims
    rng = np.random.default_rng(seed)
    ocfg = O.OracleConfig("pianoroll", *dims)
    params = O.init_params(ocfg, rng)
    for k, v in params.items():
        if k.endswith("bias") or k.endswith("beta"):
            params[k] = (0.05 * rng.standard_normal(v.shape)).astype(np.float32)
        if k.endswith("gamma"):
            params[k] = (1.0 + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    params["encoder.latent_proj.weight"][Z:] *= 0.25
    params["encoder.latent_proj.bias"][Z:] += 1.5
    cfg = model.ModelConfig(model.EncoderConfig(TransformerConfig(De, 0.2, Le, He, P), Z, C, P),
                            model.DecoderConfig(TransformerConfig(Dd, 0.2, Ld, Hd, P), Z, C, P, causal=causal), kind="pianoroll")
    m = model.Model(cfg).initialize(gpu_ctx(0), params_np=params)
    return O, ocfg, params, m, rng


class _Recorder:
    """records the symbol of every library call (ops binds _lib.call by name at import, so both names are wrapped)"""

    def __init__(self, monkeypatch):
        from musicstyletransfer_amd import _lib, ops
        self.names, real = [], _lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", call)
        monkeypatch.setattr(ops, "call", call)


def test_identity_recipe_is_the_existing_path_and_encode_stops_at_the_latent_launch(gpu, monkeypatch):
    """a = b = n, w = cw = tau = 0 on Model.encode's mu gives decoder.initial_rows' rows to within one unit in the last place of
    the activation type (the builder shares the dot product of latent_fwd.hpp but states the row's last line itself, so one
    rounding boundary may be straddled); Model.encode returns Model.__call__'s mu / sigma bit for bit, issues nothing behind the
    latent launch and leaves the training RNG stream alone"""
    from oracle import vae_oracle as O
    from musicstyletransfer_amd import ops as o
    _, ocfg, params, m, rng = _pianoroll_model(gpu)
    B, T, Z, Dd = 5, 12, 16, 32
    batch = O.synthetic_pianoroll_batch(rng, B, T, 48, num_classes=2, density=0.1, ragged=True)
    x, lens, cls = batch["x"].numpy(), batch["seq_lens"].numpy(), batch["classes"].numpy()
    rng_before = m.store.rng_state(0).clone()
    _, mu_c, sg_c = m(x, lens, cls)
    mu_c, sg_c = mu_c.clone(), sg_c.clone()
    rec = _Recorder(monkeypatch)
    mu, sigma = m.encode(x, lens, cls)
    torch.cuda.synchronize()
    names = list(rec.names)
    assert torch.equal(mu, mu_c) and torch.equal(sigma, sg_c)
    lat = [i for i, s in enumerate(names) if s.startswith("mst_latent_fwd")]
    assert len(lat) == 1 and lat[0] == len(names) - 1, names  # the latent launch is the last call: no decoder-side symbol behind it
    assert not any(s in ("mst_softmax_ce", "mst_sigmoid_bce", "mst_gemm_sigmoid_bce", "mst_loss_combine", "mst_attn_decode") for s in names)
    assert torch.equal(m.store.rng_state(0), rng_before)
    want = m.decoder.initial_rows(x, lens, cls).float()
    st = m.store
    n = torch.arange(B, dtype=torch.int32, device=gpu)
    zero = torch.zeros(B, dtype=torch.float32, device=gpu)
    c32 = torch.from_numpy(cls.astype(np.int32)).to(gpu)
    from musicstyletransfer_amd.engine import positional_table
    pos = torch.from_numpy(positional_table(Dd, 1)).to(gpu)
    z_out = torch.zeros(B, Z, device=gpu)
    dec = torch.zeros(B, Dd, dtype=st.act_dtype, device=gpu)
    o.latent_rows(mu, None, n, n, zero, c32, c32, zero, st.p("decoder.latent2hid.weight"), st.p("decoder.latent2hid.bias"),
                  st.p("decoder.class2hid.weight"), pos, float(np.sqrt(Dd)), z_out, dec)
    torch.cuda.synchronize()
    assert torch.equal(z_out, mu)
    got = dec.float()
    ulp = 2.0 ** torch.floor(torch.log2(want[:, :Dd].abs().clamp_min(2.0 ** -126))) * 2.0 ** -7  # bf16: 8 significant bits
    print("identity rows: largest difference in units in the last place:", float(((got - want[:, :Dd]).abs() / ulp).max()))
    assert ((got - want[:, :Dd]).abs() <= ulp).all()
    assert torch.equal(m.store.rng_state(0), rng_before)


def test_the_noise_is_gaussian_and_indexed_by_the_global_row(gpu):
    """moments over n = 2^18 draws within the Gaussian's own 6-sigma sampling errors (mean: 1/sqrt n; variance: sqrt(2/n); fourth
    moment: sqrt(96/n)); the draw is a function of (seed, global row, element): repeats, chunks, seeds, seed by pointer"""
    rng = np.random.default_rng(0)
    Z, Dd, N = 64, 32, 4096
    host, dev = _tables(rng, Z, Dd, 2, gpu)
    prior = dict(a=np.full(N, -1), b=np.full(N, -1), w=np.zeros(N), ca=np.zeros(N), cb=np.zeros(N), cw=np.zeros(N))
    z, rows = _rows(gpu, dev, None, None, Dd=Dd, adt=torch.bfloat16, tau=1.0, seed=5, **prior)
    e = z.astype(np.float64).reshape(-1)
    n = e.size
    assert n >= 2 ** 18
    assert abs(e.mean()) <= 6 / np.sqrt(n) and abs(e.var() - 1) <= 6 * np.sqrt(2 / n) and abs((e ** 4).mean() - 3) <= 6 * np.sqrt(96 / n)
    z2, rows2 = _rows(gpu, dev, None, None, Dd=Dd, adt=torch.bfloat16, tau=1.0, seed=5, **prior)
    assert np.array_equal(z, z2) and np.array_equal(rows, rows2)
    r, mm = 1001, 77
    part = {k: v[:mm] for k, v in prior.items()}
    z3, rows3 = _rows(gpu, dev, None, None, Dd=Dd, adt=torch.bfloat16, tau=1.0, seed=5, row0=r, **part)
    assert np.array_equal(z3, z[r: r + mm]) and np.array_equal(rows3, rows[r: r + mm])
    z4, _ = _rows(gpu, dev, None, None, Dd=Dd, adt=torch.bfloat16, tau=1.0, seed=6, **prior)
    assert not np.array_equal(z4, z)
    word = torch.tensor([5], dtype=torch.int64, device=gpu)
    z5, _ = _rows(gpu, dev, None, None, Dd=Dd, adt=torch.bfloat16, tau=1.0, seed=0, seed_ptr=word, **prior)
    assert np.array_equal(z5, z)
    z6, _ = _rows(gpu, dev, None, None, Dd=Dd, adt=torch.bfloat16, tau=0.5, seed=5, **prior)
    assert np.array_equal(z6, 0.5 * z)  # tau scales the same draw (a power of two: exactly)


def test_spherical_interpolation(gpu):
    rng = np.random.default_rng(1)
    Z, Dd = 64, 32
    host, dev = _tables(rng, Z, Dd, 2, gpu)
    u = rng.standard_normal(Z); v = rng.standard_normal(Z)
    v *= np.linalg.norm(u) / np.linalg.norm(v)
    src = np.stack([u, v, 2.5 * u, -1.5 * u, np.zeros(Z), u * (1 + 1e-7)]).astype(np.float32)
    steps = 9
    w = np.linspace(0, 1, steps).astype(np.float32)
    zero = np.zeros(steps)
    z, rows = _rows(gpu, dev, src, None, zero, zero + 1, w, zero, zero, zero, Dd, torch.bfloat16, mode="slerp")
    assert np.array_equal(z[0], src[0]) and np.array_equal(z[-1], src[1])  # the end points ARE the sources
    norms = np.linalg.norm(z.astype(np.float64), axis=1)
    n0 = np.linalg.norm(src[0].astype(np.float64))
    assert np.abs(norms / n0 - 1).max() <= 8 * Z * 2.0 ** -24, np.abs(norms / n0 - 1).max()  # equal norms stay equal (fp32 rounding)
    lin, _ = _rows(gpu, dev, src, None, zero, zero + 1, w, zero, zero, zero, Dd, torch.bfloat16, mode="lerp")
    assert not np.allclose(lin[4], z[4])  # (the spherical path is not the chord)
    for other in (2, 3, 4, 5):  # parallel, antiparallel, zero, parallel within fp32: the linear form, finite
        zs, rs = _rows(gpu, dev, src, None, zero, zero + other, w, zero, zero, zero, Dd, torch.bfloat16, mode="slerp")
        zl, rl = _rows(gpu, dev, src, None, zero, zero + other, w, zero, zero, zero, Dd, torch.bfloat16, mode="lerp")
        assert np.isfinite(zs).all() and np.isfinite(rs).all() and np.array_equal(zs, zl) and np.array_equal(rs, rl), other
        zs, _ = _rows(gpu, dev, src, None, zero + other, zero, w, zero, zero, zero, Dd, torch.bfloat16, mode="slerp")
        zl, _ = _rows(gpu, dev, src, None, zero + other, zero, w, zero, zero, zero, Dd, torch.bfloat16, mode="lerp")
        assert np.isfinite(zs).all() and np.array_equal(zs, zl), other


@pytest.mark.parametrize("adt", [torch.bfloat16, torch.float16])
def test_frame_step_draws_from_the_distribution(gpu, adt):
    """mst_frame_step, modelled on test_device_sampling_draws_from_the_distribution: N = 16384 sequences sharing one logit row"""
    from musicstyletransfer_amd import ops as o
    N, P, L, i = 16384, 45, 5, 3
    ld = 48
    g = torch.Generator().manual_seed(4)
    row = (3.0 * torch.randn(P, generator=g)).to(adt)
    row[7], row[9] = -60.0, 60.0
    logits = torch.zeros(N, ld, dtype=adt, device=gpu)
    logits[:, :P] = row.to(gpu)
    logits[:, P:] = 50.0  # pad columns of the logits must not reach the frame
    x64 = row.double().numpy()
    seed = torch.tensor([1234], dtype=torch.int64, device=gpu)

    def run(tau, mode="draw", thr=0.5, pos=i, seed_t=seed):
        frames = torch.zeros(N, ld, dtype=torch.uint8, device=gpu)
        roll = torch.zeros(N, L, ld, dtype=torch.uint8, device=gpu)
        scores = torch.full((N,), 0.5, device=gpu)
        probs = torch.zeros(N, L, P, device=gpu)
        o.frame_step(logits, P, pos, seed_t, frames, roll, scores, tau=tau, mode=mode, thr=thr, probs_out=probs)
        torch.cuda.synchronize()
        assert torch.equal(frames, roll[:, pos - 1]) and (frames[:, P:] == 0).all()  # the same frame in both places, pad columns zero
        other = [k for k in range(L) if k != pos - 1]
        assert (roll[:, other] == 0).all() and (probs[:, other] == 0).all()
        return frames[:, :P].cpu().numpy(), scores.cpu().numpy().astype(np.float64) - 0.5, probs[:, pos - 1].cpu().numpy()

    for tau in (1.0, 0.5, 2.0):
        f, sc, pr = run(tau)
        p = 1.0 / (1.0 + np.exp(-x64 / tau))
        q = 1.0 / (1.0 + np.exp(x64 / tau))
        np.testing.assert_allclose(pr[0], p, rtol=1e-5, atol=1e-30)
        counts = f.sum(0).astype(np.float64)
        sigma = np.sqrt(N * p * (1 - p)) + 1.0
        assert (np.abs(counts - N * p) <= 6 * sigma).all(), np.abs(counts - N * p).max()
        assert counts[7] == 0 and counts[9] == N
        want = -(np.log(np.maximum(np.where(f > 0, p, q), 1e-30))).sum(1)  # the likelihood of the frames actually drawn
        np.testing.assert_allclose(sc, want, rtol=1e-4, atol=1e-5)
        for thr in (0.5, 0.25, 0.8):
            ft, sct, _ = run(tau, mode="threshold", thr=thr)
            cut = np.float32(np.log(np.float64(np.float32(thr)) / (1.0 - np.float64(np.float32(thr)))))
            want_f = (logits[:, :P].float().cpu().numpy() / np.float32(tau)) > cut
            assert np.array_equal(ft > 0, want_f), (tau, thr)
            np.testing.assert_allclose(sct, -(np.log(np.maximum(np.where(ft > 0, p, q), 1e-30))).sum(1), rtol=1e-4, atol=1e-5)
    f0, _, _ = run(1.0)
    f1, _, _ = run(1.0)
    f2, _, _ = run(1.0, seed_t=torch.tensor([99], dtype=torch.int64, device=gpu))
    f3, _, _ = run(1.0, pos=i + 1)
    assert np.array_equal(f0, f1) and not np.array_equal(f0, f2) and not np.array_equal(f0, f3)
    assert not np.array_equal(f0[0], f0[1])  # sequences draw independently


@pytest.mark.parametrize("attention,causal", [("query", False), ("key", False), ("key", True)])
def test_frame_sampling_loop_is_the_host_loop(gpu, attention, causal):
    """threshold mode at 0.5 against a host loop feeding DecodePlan.step with logits > 0, position by position (B = 7, 26 positions);
    the per-position graphs are captured once and replayed for every seed"""
    from musicstyletransfer_amd import decode
    _, ocfg, params, m, rng = _pianoroll_model(gpu, causal=causal)
    st = m.store
    B, L, P, Dd = 7, 26, 48, 32
    row0 = torch.from_numpy(rng.standard_normal((B, Dd)).astype(np.float32)).to(st.act_dtype).to(gpu)
    plan = decode.DecodePlan(st, B, L, attention=attention)
    plan.start(row0)
    prev = np.zeros((B, P), np.uint8)
    prev[:, 0] = 1
    want = []
    for _ in range(1, L):
        plan.step(prev)
        torch.cuda.synchronize()
        prev = (plan.logits[:, :P].float() > 0).to(torch.uint8).cpu().numpy()
        want.append(prev)
    want = np.stack(want, 1)
    assert 0 < want.mean() < 1
    fs = m.frame_sampling_plan(B, L, attention)
    assert fs is m.frame_sampling_plan(B, L, attention)  # kept by the model
    got, scores = fs.run(row0, mode="threshold", thr=0.5, seed=1)
    assert got.shape == (B, L - 1, P) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.isfinite(scores).all() and (scores > 0).all()
    n_graphs = len(fs._graphs)
    assert n_graphs == L - 1  # one per position (the first ran eagerly and was captured behind that)
    again, _ = fs.run(row0, mode="threshold", thr=0.5, seed=2)
    assert np.array_equal(again, want) and len(fs._graphs) == n_graphs  # replayed graphs, and no random number in threshold mode
    d1, s1 = fs.run(row0, mode="draw", seed=10)
    n_draw = len(fs._graphs)
    d2, s2 = fs.run(row0, mode="draw", seed=11)
    d3, s3 = fs.run(row0, mode="draw", seed=10)
    assert len(fs._graphs) == n_draw  # another seed captures nothing
    assert not np.array_equal(d1, d2) and np.array_equal(d1, d3) and np.array_equal(s1, s3)
    short, _ = fs.run(row0, length=9, mode="draw", seed=10)
    assert short.shape == (B, 8, P) and np.array_equal(short, d1[:, :8])
    with pytest.raises(ValueError):
        fs.run(row0, length=L + 1)


@pytest.mark.parametrize("attention", ["query", "key"])
def test_transfer_matches_the_oracle(gpu, attention):
    """the restyled melody is the decoder's output for (z of the source, class of the target): on the piano-roll model and sizes of
    test_decode_step_matches_the_oracle (B 5, 9 positions), greedy transfer to the other class with the per-position probabilities
    kept; oracle.decode_incremental fed the start frame and the returned roll reproduces them within that test's tolerance (mean
    error <= 3e-3, largest <= 6e-2). Every row and position is compared."""
    from musicstyletransfer_amd import generate as G
    from music_style_transfer.VarAutoEncoder.data import Batch
    O, ocfg, params, m, rng = _pianoroll_model(gpu)
    B, T, n, P = 5, 12, 9, 48
    batch = O.synthetic_pianoroll_batch(rng, B, T, P, num_classes=2, density=0.1, ragged=True)
    x, lens, cls = batch["x"].numpy(), batch["seq_lens"].numpy(), batch["classes"].numpy()
    gen = G.LatentGenerator(m, attention=attention, decoder="greedy", keep_probs=True)
    one = Batch([x, lens, cls], [])
    mu, _ = gen.encode(one)
    res = gen.transfer(one, [0, 1], length=n + 1)
    keep = [r for r in range(len(res)) if res.rows[r]["cls"] == 1 - cls[res.rows[r]["melody"]]]
    assert len(keep) == B and [res.rows[r]["melody"] for r in keep] == list(range(B))
    z, roll, probs = res.z[keep], res.rolls[keep], res.probs[keep]
    assert np.array_equal(z, mu.cpu().numpy())  # z of the source
    assert roll.shape == (B, n, P) and probs.shape == (B, n, P) and np.array_equal(roll, (probs > 0.5).astype(np.uint8))
    target = 1 - cls
    start = np.zeros((B, 1, P), np.uint8)
    start[:, 0, 0] = 1
    fed = np.concatenate([start, roll[:, : n - 1]], 1)  # position t + 1 is fed frame t; position 1 the start row
    Pm = O.to_torch_params(m.store.as_consumed_numpy(), requires_grad=False)
    want = O.decode_incremental(Pm, ocfg, torch.from_numpy(z), torch.from_numpy(target), torch.from_numpy(fed), attention).numpy()
    err = np.abs(probs - want)
    print("transfer vs oracle: mean", err.mean(), "max", err.max())
    assert err.mean() <= 3e-3 and err.max() <= 6e-2, (err.mean(), err.max())


def test_interface_on_the_toy_model(gpu, tmp_path, monkeypatch):
    from music_style_transfer.VarAutoEncoder import main, sampler as S, utils
    from music_style_transfer.VarAutoEncoder import generate as G
    from music_style_transfer.VarAutoEncoder.data import ToyData
    from music_style_transfer.MIDIUtil import smf

    class A:
        verbose, beam_size = False, 3

    t = main.main(["--toy", "--gpu", "--max-steps", "300", "--model-output", str(tmp_path)])
    t.stream.synchronize()
    torch.cuda.synchronize()
    batch = next(iter(ToyData()))
    rec = _Recorder(monkeypatch)
    smp = S.get_sampler("sampling", None, None, None, A)
    smp.update_parameters(t.model)
    old = smp.process_batch(batch, str(tmp_path / "old"), 3)
    n_old = sum(s.startswith("mst_latent_fwd") for s in rec.names)
    del rec.names[:]
    tr = S.get_sampler("transfer", None, None, None, A)
    tr.update_parameters(t.model)
    new = tr.process_batch(batch, str(tmp_path / "new"), 3)
    n_new = sum(s.startswith("mst_latent_fwd") for s in rec.names)
    assert (n_old, n_new) == (3, 1)  # one encoder pass instead of one per class
    assert len(new) == 3 + 3 * 3 and [os.path.basename(f) for f in new] == [os.path.basename(f) for f in old]
    assert all(os.path.getsize(f) > 0 for f in new)
    assert "mst_latent_rows" in rec.names and rec.names.count("mst_latent_rows") == 1
    for name in ("prior", "interpolation"):
        s2 = S.get_sampler(name, None, None, None, A)
        s2.update_parameters(t.model)
        files = s2.process_batch(batch, str(tmp_path / name), 3)
        assert len(files) == (9 if name == "prior" else 16) and all(os.path.getsize(f) > 0 for f in files)

    for decoder in ("sampling", "greedy", "beam"):
        gen = G.LatentGenerator(t.model, seed=3, decoder=decoder, max_rows=4)
        pr = gen.prior(5, [0, 1, 2, 0, 1], 10)  # (two chunks: 4 + 1 rows)
        assert pr.z.shape == (5, 16) and pr.sequences.shape == (5, 10) and pr.scores.shape == (5,) and np.isfinite(pr.scores).all()
        assert ((pr.sequences >= 0) & (pr.sequences < 10)).all() and (pr.sequences[:, 0] == 1).all() and len(pr.rows) == 5
        assert np.abs(pr.z).max() > 0 and np.isfinite(pr.z).all()
        it = gen.interpolate(batch, 0, 2, steps=7)
        assert it.z.shape == (7, 16) and it.sequences.shape == (7, 10) and np.isfinite(it.scores).all()
        assert ((it.sequences >= 0) & (it.sequences < 10)).all() and [r["cls"] for r in it.rows] == [0, 0, 0, 0, 2, 2, 2]
        tf = gen.transfer(batch)
        assert tf.z.shape == (9, 16) and tf.sequences.shape == (9, 10)
        first = [r for r in range(9) if tf.rows[r] == dict(melody=0, cls=0)][0]
        last = [r for r in range(9) if tf.rows[r] == dict(melody=2, cls=2)][0]
        # the end points of the interpolation are the two melodies themselves: the same z, the same decoder start rows
        assert np.array_equal(it.z[0], tf.z[first]) and np.array_equal(it.z[6], tf.z[last])
        assert torch.equal(it.start_rows[0], tf.start_rows[first]) and torch.equal(it.start_rows[6], tf.start_rows[last])
        bl = gen.class_blend(batch, 0, 2, [0.0, 0.5, 1.0])
        assert bl.z.shape == (9, 16) and bl.sequences.shape == (9, 10) and np.isfinite(bl.scores).all()
        assert ((bl.sequences >= 0) & (bl.sequences < 10)).all()
        assert torch.equal(bl.start_rows[0], tf.start_rows[first])        # weight 0: class_a's embedding itself
        assert np.array_equal(bl.z[:3], np.repeat(tf.z[first: first + 1], 3, 0))
        po = gen.posterior(batch, 4)
        assert po.z.shape == (12, 16) and po.sequences.shape == (12, 10) and not np.array_equal(po.z[0], po.z[1])
    # chunked and unchunked generators with one seed draw the same latent vectors
    za = G.LatentGenerator(t.model, seed=8, max_rows=2).prior(5, 0, 6).z
    zb = G.LatentGenerator(t.model, seed=8, max_rows=64).prior(5, 0, 6).z
    assert np.array_equal(za, zb)

    # the command line: a saved checkpoint -> .mid files that read back
    folder = os.path.join(str(tmp_path), "model")
    utils.save_model(t.model, os.path.join(folder, "params.0"))
    for mode, n_files in (("transfer", 9), ("prior", 4), ("interpolate", 5), ("posterior", 6), ("blend", 15)):
        out = str(tmp_path / ("cli-" + mode))
        files = G.main(["--model-output", folder, "--checkpoint", "-1", "--mode", mode, "--toy", "--n", "4" if mode == "prior" else "2",
                        "--steps", "5", "--pair", "0", "2", "--length", "10", "--decoder", "greedy", "--seed", "1", "--out", out])
        assert len(files) == n_files and sorted(os.listdir(out)) == sorted(os.path.basename(f) for f in files)
        for f in files:
            assert os.path.getsize(f) > 0
            assert len(list(smf.read_midifile(f))) == 1  # one track, parseable
    assert os.path.exists(os.path.join(str(tmp_path), "cli-transfer", "transfer-1.class-2.mid"))
    assert os.path.exists(os.path.join(str(tmp_path), "cli-interpolate", "interp-0-2.04.mid"))
