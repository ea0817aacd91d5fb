"""Clipping by the global gradient norm on the device: the sum-of-squares launch against fp64 (tests/clip_refs.py), the
gnorm form of the Adam launch against the plain launches handed the factor — bit for bit, since it is the plain launch with
fl32(rescale * c) in place of rescale —, the skip of a step whose norm is not finite, and whole steps, eager and captured."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import clip_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
DIMS = (128, 128, 3, 32, 64, 1, 4, 64, 2, 4)  # the small model of tests/test_schedule_gpu.py
B_STEP, T_STEP = 4, 33
N_BIG = 2 ** 21 + 3
LO, HI = 1 / 64, 1 / 65536  # two rescales, both exact in fp32
_bucket = {}


def ops():
    from musicstyletransfer_amd import ops as o
    return o


def _big():
    """one random bucket of N_BIG values (scale 50) for every size of the sum-of-squares tests; made once, never written"""
    if "g" not in _bucket:
        _bucket["g"] = (torch.randn(N_BIG, generator=torch.Generator().manual_seed(2024)) * 50).float()
        _bucket["g64"] = _bucket["g"].numpy().astype(np.float64)
    return _bucket["g"], _bucket["g64"]


def _sumsq(o, g, cut, lo, hi):
    parts = torch.full((o.grad_sumsq_parts(),), -1.0, device=g.device)  # (every workgroup must write its part)
    o.grad_sumsq(g, cut, lo, hi, parts)
    torch.cuda.synchronize()
    return parts


def _cuts(n):
    b = n // 2 // 4 * 4
    return sorted({0, n} | {c for c in (b + 1, b + 2, b + 3) if c <= n})


# ------------------------------------------------------------------------------------------ 1. sum of squares against fp64
@pytest.mark.parametrize("n", [1, 3, 4, 255, 1027, 65537, N_BIG])
def test_grad_sumsq_against_fp64(gpu, n):
    """Tolerance (clip_refs.sumsq_bound), derived: all terms are non-negative, so the error of the fp32 sum relative to the exact sum is
    at most (number of roundings on the longest path) * 2^-24: the per-thread chain L = ceil(n / (G * 256)), plus 16 for the two
    multiplications of a term, six DPP levels, the LDS sum and slack. The parts themselves are added in fp64 here."""
    o = ops()
    G = o.grad_sumsq_parts()
    assert 0 < G <= 256
    g_cpu, g64 = _big()
    g = g_cpu[:n].to(gpu)
    cuts = _cuts(n)
    assert {0, n} <= set(cuts) and (n < 3 or {c % 4 for c in cuts} >= {1, 2, 3})
    for cut in cuts:
        parts = _sumsq(o, g, cut, LO, HI).cpu().numpy().astype(np.float64)
        want = R.sumsq(g64[:n], cut, LO, HI)
        got = float(parts.sum())
        assert (parts >= 0).all() and np.isfinite(parts).all()
        err, tol = abs(got - want) / want, R.sumsq_bound(n, G)
        print(f"n {n} cut {cut}: sum of parts {got:.9g}, fp64 {want:.9g}, relative error {err:.3g} (bound {tol:.3g})")
        assert err <= tol, (n, cut, got, want, err, tol)


# ------------------------------------------------------------------------------------------ 2. exact case, repeatability
def test_grad_sumsq_exact_and_repeatable(gpu):
    o = ops()
    G = o.grad_sumsq_parts()
    g = torch.zeros(N_BIG, device=gpu)
    g[0], g[N_BIG - 1] = 3.0, 4.0  # the first workgroup's first vector; the scalar tail
    parts = _sumsq(o, g, N_BIG // 2 + 1, 1.0, 1.0)
    assert float(parts.double().sum()) == 25.0
    nz = parts.nonzero().flatten().tolist()
    assert nz == [0, G - 1] and parts[0].item() == 9.0 and parts[G - 1].item() == 16.0
    # two launches on the same data: the same bits
    g_cpu, _ = _big()
    r = g_cpu.to(gpu)
    a, b = _sumsq(o, r, N_BIG // 2 + 3, LO, HI), _sumsq(o, r, N_BIG // 2 + 3, LO, HI)
    assert torch.equal(a, b) and (a > 0).all()


# ------------------------------------------------------------------------------------------ Adam launches: helpers
LR, T0 = 1e-3, 5
EMB = (64, 0, 10, 32)  # a [10, 32] matrix at flat offset 64 whose transposed shadow the launch keeps (mst_adam_args.emb)


def _problem(gpu, n, seed):
    g = torch.Generator().manual_seed(seed)
    p = dict(w=torch.randn(n, generator=g), grad=torch.randn(n, generator=g) * 50, m=torch.randn(n, generator=g) * 0.1,
             v=torch.rand(n, generator=g) * 0.01, recon=torch.rand(7, generator=g) * 20, kl=torch.rand(7, generator=g) * 8)
    return {k: t.to(gpu) for k, t in p.items()}


def _fresh(gpu, p, dtype, t=T0, lo=0, hi=None):
    """the state one launch over [lo, hi) updates: clones of w, m, v, zeroed shadows, a step state as step_begin leaves it"""
    hi = p["w"].numel() if hi is None else hi
    s = dict(w=p["w"][lo:hi].clone(), m=p["m"][lo:hi].clone(), v=p["v"][lo:hi].clone(), w16=torch.zeros(hi - lo, dtype=dtype, device=gpu),
             wt16=torch.zeros(32 * 16, dtype=dtype, device=gpu), total=torch.zeros(7, device=gpu), metric=torch.zeros(3, device=gpu),
             state=torch.tensor([t, 0], dtype=torch.int32, device=gpu))
    s["state"].view(torch.float32)[1] = LR
    return s


def _launch(o, p, s, rescale, variant, lo=0, hi=None, gnorm=None, wd=0.0, clip=-1.0, status=None, books=True):
    """one Adam launch over [lo, hi) of problem p on state s; variant: which of emb / sched ride along"""
    hi = p["w"].numel() if hi is None else hi
    emb = dict(base=lo, specs=[EMB], wt16=s["wt16"]) if "emb" in variant else None
    sched = p["sched"] if "sched" in variant and books else None
    guard = dict(status=status, expect=[]) if status is not None else {}
    if books:
        mt = dict(recon=p["recon"], kl=p["kl"], kl_weight=0.5, total=s["total"], metric=s["metric"], **guard)
    else:
        mt = guard or None
    o.adam_flat(s["w"], p["grad"][lo:hi], s["m"], s["v"], s["w16"], s["state"], lr=LR, rescale=rescale, clip=clip, wd=wd, advance_step=False,
                metrics=mt, emb=emb, sched=sched, gnorm=gnorm)
    torch.cuda.synchronize()
    return s


def _same(a, b, what):
    for k in ("w", "m", "v", "w16", "wt16", "total", "metric", "state"):
        assert torch.equal(a[k], b[k]), (what, k)


def _ulps(a, b):
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(b)))


# ------------------------------------------------------------------------------------------ 3. unclipped
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [5, 3074])
def test_adam_gnorm_unclipped_is_the_plain_launch(gpu, n, dtype):
    o = ops()
    p = _problem(gpu, n, 11 + n)
    r = 1 / 32
    parts = _sumsq(o, p["grad"], 0, r, r)
    norm64 = math.sqrt(R.sumsq(p["grad"].cpu().numpy(), 0, r, r))
    gstat = torch.zeros(8, device=gpu)
    for wd, clip in ((0.0, -1.0), (0.01, 0.5)):
        gstat.zero_()
        a = _launch(o, p, _fresh(gpu, p, dtype), r, "plain", wd=wd, clip=clip,
                    gnorm=dict(parts=parts, max_norm=float(np.float32(2 * norm64)), gstat=gstat))
        b = _launch(o, p, _fresh(gpu, p, dtype), r, "plain", wd=wd, clip=clip)
        _same(a, b, (wd, clip))
        assert not torch.equal(a["w"], p["w"]) and torch.equal(a["w16"], a["w"].to(dtype)) and int(a["state"][0]) == T0
        gs = gstat.cpu().numpy()
        assert gs[1] == 1.0 and _ulps(gs[0], norm64) <= 2 + R.sumsq_bound(n, parts.numel()) * 2 ** 23
        assert gs[2] == gs[0] == gs[3] and gs[4] == 1.0 and gs[5] == 0.0 and not gs[6:].any()


# ------------------------------------------------------------------------------------------ 4. clipped
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("variant,n", [("plain", 5), ("plain", 3074), ("emb", 3074), ("sched", 3074), ("emb_sched", 3074)])
def test_adam_gnorm_clipped_is_the_plain_launch_at_the_scaled_rescale(gpu, variant, n, dtype):
    from musicstyletransfer_amd import engine as E
    o = ops()
    p = _problem(gpu, n, 23 + n)
    p["sched"] = torch.tensor([0.375, 3.0, 1.0, 6.0], device=gpu)
    r = 1 / 32
    parts = _sumsq(o, p["grad"], 0, r, r)
    norm64 = math.sqrt(R.sumsq(p["grad"].cpu().numpy(), 0, r, r))
    max_norm = float(np.float32(0.5 * norm64))  # the decision c < 1 is far from any rounding
    for wd, clip in ((0.0, -1.0), (0.01, 0.05)):
        gstat = torch.zeros(8, device=gpu)
        a = _launch(o, p, _fresh(gpu, p, dtype), r, variant, wd=wd, clip=clip, gnorm=dict(parts=parts, max_norm=max_norm, gstat=gstat))
        norm, c = gstat.cpu().numpy()[:2]
        assert c.tobytes() == E.clip_scale(norm, max_norm).tobytes() and 0.49 < c < 0.51
        assert _ulps(norm, math.sqrt(float(parts.double().sum()))) <= 2
        scaled = float(np.float32(r) * np.float32(c))  # rounded once
        b = _launch(o, p, _fresh(gpu, p, dtype), scaled, variant, wd=wd, clip=clip)
        _same(a, b, (variant, wd, clip))
        assert torch.equal(a["w16"], a["w"].to(dtype)) and a["metric"][2].item() == 7
        if "emb" in variant:
            so, _, rows, cols = EMB
            assert torch.equal(a["wt16"].view(cols, 16)[:, :rows], a["w"][so:so + rows * cols].view(rows, cols).t().to(dtype))
        if clip >= 0 and n > 100:  # the per-element clip is reached by some elements and not by all
            gg = (p["grad"] * scaled + wd * p["w"]).abs()
            assert (gg > clip).any() and (gg < clip).any()
        if clip < 0 or n > 100:  # (five elements may all sit on the per-element bound with and without the factor)
            unscaled = _launch(o, p, _fresh(gpu, p, dtype), r, variant, wd=wd, clip=clip)
            assert not torch.equal(a["m"], unscaled["m"])
        assert gstat.cpu().tolist()[2:6] == [float(norm), float(norm), 1.0, 1.0]


# ------------------------------------------------------------------------------------------ 5. three steps against fp64
def test_adam_gnorm_three_steps_against_fp64(gpu):
    """test_adam_flat_mxnet_rule's problem and tolerances, with a bound that clips every step (norms near 156 against 50)"""
    from test_kernels_gpu import close, rnd
    o = ops()
    n, lr, r, max_norm, b1, b2 = 10007, 3e-4, 1 / 32, 50.0, 0.9, 0.999
    w = rnd((n,), gpu, dtype=torch.float32, seed=100)
    m, v, w16 = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu), torch.zeros(n, dtype=BF, device=gpu)
    state = torch.zeros(2, dtype=torch.int32, device=gpu)
    parts, gstat = torch.zeros(o.grad_sumsq_parts(), device=gpu), torch.zeros(8, device=gpu)
    wr, mr, vr = w.cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 4):
        g = rnd((n,), gpu, dtype=torch.float32, seed=100 + t, scale=50.0)
        state[0] = t  # what the step's first launch does: the count and the bias-corrected rate, evaluated in double
        state.view(torch.float32)[1] = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        o.grad_sumsq(g, 0, r, r, parts)
        o.adam_flat(w, g, m, v, w16, state, lr=lr, rescale=r, clip=1.0, advance_step=False, gnorm=dict(parts=parts, max_norm=max_norm, gstat=gstat))
        g64 = g.cpu().numpy().astype(np.float64)
        norm, c = R.norm_and_scale(R.sumsq(g64, 0, r, r), max_norm)
        assert c < 0.5
        wr, mr, vr = R.adam_step(wr, g64, mr, vr, t, lr, b1, b2, 1e-8, 0.0, r, 1.0, c)
        torch.cuda.synchronize()
        assert abs(gstat[0].item() - norm) <= 1e-6 * norm and abs(gstat[1].item() - c) <= 1e-6 * c
    assert gstat.cpu().tolist()[4:6] == [3.0, 3.0] and state[0].item() == 3
    close(w, torch.from_numpy(wr), 1e-6, 1e-7, "adam w")
    close(m, torch.from_numpy(mr), 1e-5, 1e-7, "adam m")
    close(v, torch.from_numpy(vr), 1e-4, 1e-9, "adam v")
    assert torch.equal(w16, w.to(BF))


# ------------------------------------------------------------------------------------------ 6. two ranges
N2, CUT2, R_LO, R_HI = 3074, 1540, 1 / 4, 1 / 4096  # the fp16 layout: two loss-scale ranges, the cut a multiple of 4


def test_two_ranges_apply_the_same_factor(gpu):
    from musicstyletransfer_amd import engine as E
    o = ops()
    p = _problem(gpu, N2, 61)
    p["grad"][CUT2:] *= 1024  # (the decoder side carries the loss scale)
    parts = _sumsq(o, p["grad"], CUT2, R_LO, R_HI)
    norm64 = math.sqrt(R.sumsq(p["grad"].cpu().numpy(), CUT2, R_LO, R_HI))
    max_norm = float(np.float32(0.5 * norm64))
    gstat = torch.zeros(8, device=gpu)
    gn = dict(parts=parts, max_norm=max_norm)
    a0 = _launch(o, p, _fresh(gpu, p, F16, hi=CUT2), R_LO, "emb", hi=CUT2, gnorm=dict(gstat=gstat, **gn))
    a1 = _launch(o, p, _fresh(gpu, p, F16, lo=CUT2), R_HI, "emb", lo=CUT2, gnorm=gn, books=False)
    norm, c = gstat.cpu().numpy()[:2]
    assert c.tobytes() == E.clip_scale(norm, max_norm).tobytes() and _ulps(norm, norm64) <= 2 + R.sumsq_bound(N2, parts.numel()) * 2 ** 23
    b0 = _launch(o, p, _fresh(gpu, p, F16, hi=CUT2), float(np.float32(R_LO) * c), "emb", hi=CUT2)
    b1 = _launch(o, p, _fresh(gpu, p, F16, lo=CUT2), float(np.float32(R_HI) * c), "emb", lo=CUT2, books=False)
    _same(a0, b0, "range 0")
    _same(a1, b1, "range 1")
    assert gstat[4].item() == 1.0 and not torch.equal(a1["w"], p["w"][CUT2:])


# ------------------------------------------------------------------------------------------ 7. non-finite gradient
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_nonfinite_gradient_skips_the_step_once(gpu, bad):
    """a NaN / inf in the bucket is data for the guard: it reaches Adam's launches only through the norm, which skips them"""
    o = ops()
    p = _problem(gpu, N2, 71)
    clean = p["grad"].clone()
    status = torch.zeros(3, dtype=torch.int32, device=gpu)
    gstat = torch.full((8,), 7.0, device=gpu)
    parts = torch.zeros(o.grad_sumsq_parts(), device=gpu)
    s0, s1 = _fresh(gpu, p, F16, t=T0, hi=CUT2), _fresh(gpu, p, F16, t=T0, lo=CUT2)
    s1["state"] = s0["state"]  # one step state for both ranges, as in a step
    before = [{k: t.clone() for k, t in s.items()} for s in (s0, s1)]

    def step():
        s0["state"][0] += 1  # (the step's first launch advances the count)
        o.grad_sumsq(p["grad"], CUT2, R_LO, R_HI, parts)
        gn = dict(parts=parts, max_norm=1.0)
        _launch(o, p, s0, R_LO, "emb", hi=CUT2, gnorm=dict(gstat=gstat, **gn), status=status)
        _launch(o, p, s1, R_HI, "emb", lo=CUT2, gnorm=gn, status=status, books=False)

    for k, where in enumerate((CUT2 + 77, 5, N2 - 1), 1):  # in the second range, in the first, in the scalar tail
        p["grad"].copy_(clean)
        p["grad"][where] = bad
        step()
        assert not torch.isfinite(parts).all()
        for s, b in zip((s0, s1), before):
            _same(s, b, (where, "skipped"))  # (the state word too: the count was taken back)
        assert status.tolist() == [0, 0, k] and gstat.cpu().tolist() == [7.0] * 8
    # the next clean step counts
    p["grad"].copy_(clean)
    step()
    assert torch.isfinite(parts).all() and status.tolist() == [0, 0, 3]
    assert int(s0["state"][0]) == T0 + 1 and s0["metric"][2].item() == 7
    assert not torch.equal(s0["w"], before[0]["w"]) and not torch.equal(s1["w"], before[1]["w"])
    gs = gstat.cpu().tolist()
    assert gs[4] == 8.0 and gs[5] == 8.0 and gs[6:] == [7.0, 7.0] and gs[1] < 1 and gs[0] > 1
    # without status words the update is skipped all the same, only not counted
    p["grad"][3] = bad
    s = _fresh(gpu, p, BF, t=T0 + 1)
    o.grad_sumsq(p["grad"], 0, R_LO, R_LO, parts)
    _launch(o, p, s, R_LO, "plain", gnorm=dict(parts=parts, max_norm=1.0, gstat=gstat), books=False)
    assert torch.equal(s["w"], p["w"]) and torch.equal(s["m"], p["m"]) and torch.equal(s["v"], p["v"]) and not s["w16"].any()
    assert int(s["state"][0]) == T0 and gstat.cpu().tolist() == gs and status.tolist() == [0, 0, 3]


# ------------------------------------------------------------------------------------------ 8. whole steps
def _small_step(gpu, dtype, seed=13, **hyper):
    """store + plan of the small piano-roll model on a full-length batch (explicit eps, dropout 0), on the LayerNorm-backward form whose
    sums have a fixed order (LN_PARTIALS_MIN = 0: DESIGN §11, "Where bit-identity is asserted")"""
    from test_step_gpu import _setup
    O, E, ocfg, ecfg, params, batch, eps = _setup("pianoroll", DIMS, B_STEP, T_STEP, seed, ragged=False)
    store = E.ParamStore(ecfg, gpu, dtype, params_np=params)
    plan = E.StepPlan(store, B_STEP, T_STEP, clip_gradient=1.0, lr=1e-3, **hyper)
    plan.LN_PARTIALS_MIN = 0
    plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
    return E, store, plan


def _norm_ref(store, plan):
    """fp64 norm of the bucket as the optimizer is about to read it, at the rescales of its launches"""
    cut = store.offsets["decoder.latent2hid.weight"] if plan.gscale != plan.gscale_enc else 0
    return math.sqrt(R.sumsq(store.g.cpu().numpy(), cut, 1.0 / (plan.global_batch * plan.gscale_enc), 1.0 / (plan.global_batch * plan.gscale)))


def _captured(store, plan):
    from test_schedule_gpu import _restore, _state
    saved = _state(store)
    plan.step_kernels(True)  # (HIP modules load lazily and are not capturable)
    torch.cuda.synchronize()
    plan.capture(True)
    _restore(store, saved)


@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
def test_whole_steps_off_path_call_list_nodes_and_replays(gpu, dtype):
    from test_schedule_gpu import _calls
    o = ops()
    E, s_off, p_off = _small_step(gpu, dtype)
    _, s_zero, p_zero = _small_step(gpu, dtype, clip_global_norm=0.0)
    _, s_on, p_on = _small_step(gpu, dtype, clip_global_norm=1e6)  # never clips
    assert not p_off.forms.gnorm and not p_zero.forms.gnorm and p_on.forms.gnorm
    two = dtype == F16
    assert (p_on.gscale != p_on.gscale_enc) == two  # fp16: the two-range form
    # (a) the call lists
    from test_schedule_gpu import _restore, _state
    saved = [(s, _state(s)) for s in (s_off, s_zero, s_on)]
    names = {k: _calls(o, lambda: p.step_kernels(True)) for k, p in (("off", p_off), ("zero", p_zero), ("on", p_on))}
    torch.cuda.synchronize()
    adam = [i for i, nm in enumerate(names["off"]) if nm.startswith("mst_adam_flat")]
    assert names["off"] == names["zero"] and not any(nm == "mst_grad_sumsq" or "+gnorm" in nm for nm in names["off"])
    assert len(adam) == (2 if two else 1) and adam == list(range(adam[0], adam[0] + len(adam)))
    assert {names["off"][i] for i in adam} <= {"mst_adam_flat", "mst_adam_flat+emb"}
    want = list(names["off"])
    for i in adam:
        want[i] = names["off"][i] + "+gnorm"  # (the same launch otherwise: the matrices it keeps included)
    want.insert(adam[0], "mst_grad_sumsq")
    assert names["on"] == want
    assert "grad_norm" not in s_off.read_metrics(reset=False) and not s_off.gstat.any()
    assert set(p_off.metrics(reset=False)) == set(p_on.metrics(reset=False)) - {"grad_norm", "grad_norm_max", "clip_frac"}
    for s, was in saved:
        _restore(s, was)
    # (b), (c): captured; one kernel node more; six replays bit-identical to the option off, the norm reported after each
    n, G = s_on.n, o.grad_sumsq_parts()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
        for s, p in ((s_off, p_off), (s_on, p_on)):
            _captured(s, p)
        assert torch.equal(s_off.w, s_on.w) and torch.equal(s_off.wt16, s_on.wt16) and int(s_on.step_state[0]) == 0
        (n_off, k_off), (n_on, k_on) = p_off.graph_nodes(), p_on.graph_nodes()
        assert (n_on, k_on) == (n_off + 1, k_off + 1), (p_off.graph_nodes(), p_on.graph_nodes())
        norms = []
        for t in range(1, 7):
            p_off.run()
            p_on.run()
            torch.cuda.synchronize()
            assert torch.equal(s_off.w, s_on.w) and torch.equal(s_off.m, s_on.m) and torch.equal(s_off.v, s_on.v), t
            assert torch.equal(s_off.w16, s_on.w16) and torch.equal(s_off.wt16, s_on.wt16)
            assert int(s_on.step_state[0]) == int(s_off.step_state[0]) == t
            m = s_on.read_metrics(reset=True)
            want_norm = _norm_ref(s_on, p_on)
            # item 1's bound holds for S; the norm halves it, and sqrtf and the conversion to fp32 add two roundings: still inside it
            assert abs(m["grad_norm"] - want_norm) <= R.sumsq_bound(n, G) * want_norm, (t, m["grad_norm"], want_norm)
            assert m["grad_norm_max"] == m["grad_norm"] and m["clip_frac"] == 0.0 and s_on.gstat[1].item() == 1.0
            norms.append(m["grad_norm"])
        assert "grad_norm" not in s_on.read_metrics(reset=False)  # (reset cleared the running fields)
        # (d) a bound at half the first step's norm
        _, s_clip, p_clip = _small_step(gpu, dtype, clip_global_norm=0.5 * norms[0])
        _captured(s_clip, p_clip)
        assert p_clip.graph_nodes() == p_on.graph_nodes()
        for t in range(1, 7):
            p_clip.run()
            torch.cuda.synchronize()
            assert int(s_clip.step_state[0]) == t
        m = p_clip.metrics(reset=False)
        assert m["clip_frac"] > 0 and m["grad_norm_max"] >= m["grad_norm"] > 0 and m["count"] == 6 * B_STEP and m["nonfinite_steps"] == 0
        assert not torch.equal(s_clip.w, s_on.w) and torch.isfinite(s_clip.w).all()
        assert s_clip.read_metrics(reset=False)["grad_norm"] == m["grad_norm"] and int(s_clip.step_status.cpu()[1]) == 0


# ------------------------------------------------------------------------------------------ 9. the data-parallel guard, on one GPU
def test_data_parallel_guard_skips_on_a_nonfinite_reduced_bucket(gpu):
    """global_batch = 2 B: the plan carries no loss check (StepPlan._guard), the norm of the reduced bucket is the guard. The three-graph
    data-parallel form, with a stand-in for the all-reduce that writes a NaN into the bucket between the graphs."""
    from test_step_gpu import _setup
    dims, B, T = (32, 32, 2, 16, 32, 2, 2, 32, 1, 2), 4, 16  # two encoder layers: grad_cut() > 0, three graphs
    O, E, ocfg, ecfg, params, batch, eps = _setup("pianoroll", dims, B, T, 37)
    plans = []
    with torch.cuda.stream(torch.cuda.Stream()):
        for max_norm in (0.0, 1e6):
            store = E.ParamStore(ecfg, gpu, BF, params_np=params)
            plan = E.StepPlan(store, B, T, lr=1e-3, global_batch=2 * B, clip_global_norm=max_norm)
            assert "finite" not in plan._guard()
            plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
            plan.step_kernels(True)
            torch.cuda.synchronize()
            plan.capture(True, split_optimizer=True, overlap=True)
            assert plan.graph_late is not None and plan.grad_cut() > 0
            plans.append((store, plan))
        (s_off, p_off), (store, plan) = plans
        # the sum-of-squares node sits in the optimizer's graph, behind the all-reduce
        assert plan.graph_opt.kernel_nodes == p_off.graph_opt.kernel_nodes + 1
        assert plan.graph.kernel_nodes == p_off.graph.kernel_nodes and plan.graph_late.kernel_nodes == p_off.graph_late.kernel_nodes
        store.read_metrics(reset=True)
        w, m, v, w16 = (t.clone() for t in (store.w, store.m, store.v, store.w16))
        t0 = int(store.step_state[0])

        def poison(flat):
            flat[flat.numel() // 3] = float("nan")

        plan.run(reduce_fn=poison)
        torch.cuda.synchronize()
        assert torch.equal(store.w, w) and torch.equal(store.m, m) and torch.equal(store.v, v) and torch.equal(store.w16, w16)
        assert int(store.step_state[0]) == t0
        before = store.nonfinite_steps
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            got = store.read_metrics(reset=True)
        assert got["nonfinite_steps"] == 1 and store.nonfinite_steps == before + 1 and got["count"] == 0 and "grad_norm" not in got
        assert any("skipped" in str(x.message) for x in seen)
        plan.run(reduce_fn=lambda flat: None)  # an identity all-reduce: the step counts
        torch.cuda.synchronize()
        got = store.read_metrics(reset=True)
        assert int(store.step_state[0]) == t0 + 1 and not torch.equal(store.w, w) and torch.isfinite(store.w).all()
        assert got["nonfinite_steps"] == 0 and got["count"] == B and got["grad_norm"] > 0 and got["clip_frac"] == 0.0


# ------------------------------------------------------------------------------------------ 10. the trainer
def test_trainer_logs_the_norm_only_when_the_option_is_on(gpu, tmp_path):
    from music_style_transfer.VarAutoEncoder import main
    t = main.main(["--toy", "--gpu", "--max-steps", "3", "--clip-global-norm", "0.05", "--model-output", str(tmp_path / "on")])
    assert t.config.clip_global_norm == 0.05 and t.hyper["clip_global_norm"] == 0.05 and t._last_plan.forms.gnorm
    got = t.collect_metrics(reset=False)
    assert {"grad_norm", "grad_norm_max", "clip_frac", "kl_weight", "lr_scale", "kl_loss", "total_loss"} <= set(got)
    assert got["grad_norm_max"] >= got["grad_norm"] > 0 and 0 <= got["clip_frac"] <= 1 and int(t.model.store.step_state[0].item()) == 3
    line = t._metric_to_string_output(3)
    assert "grad_norm=" in line and "grad_norm_max=" in line and "clip_frac=" in line and "kl_weight=" in line
    t = main.main(["--toy", "--gpu", "--max-steps", "3", "--model-output", str(tmp_path / "off")])
    assert "clip_global_norm" not in t.hyper and not t._last_plan.forms.gnorm
    assert set(t.collect_metrics(reset=False)) == set(got) - {"grad_norm", "grad_norm_max", "clip_frac"}
