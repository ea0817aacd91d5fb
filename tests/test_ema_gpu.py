"""The exponential moving average of the weights inside the captured step: the averaging form of the Adam launch against the
existing entry point of the same form (w, m, v and the shadows bit for bit) and against the host statement of the rule (engine.ema_update
at engine.ema_decay_at, bit for bit: the kernel's two rounded products and one rounded sum are np.float32's), the launches the guards skip,
the exchange launch, whole steps eager and captured, and the trainer: checkpoint, resume, validation and generate.py --ema."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BF, F16 = torch.bfloat16, torch.float16
DIMS = (128, 128, 3, 32, 64, 1, 4, 64, 2, 4)  # the small model of tests/test_clip_gpu.py
B_STEP, T_STEP = 4, 33
# the scalar tail alone (twice), a single workgroup with a vector part, several workgroups — and, since a launch has up to 2048 workgroups
# of 256 threads and a four-vector a thread and round, the smallest kind of size at which threads take a second grid-stride round
SIZES = [1, 3, 1023, 256 * 1024 + 5, 2 ** 21 + 1027]
DECAY = 0.99
STEPS = (1, 7, 889, 890, 5000)  # t = 1, inside the warm-up, the last step below the crossing of 0.99, the crossing, far beyond
LR, R = 1e-3, 1 / 32
EMB = (64, 0, 10, 32)  # a [10, 32] matrix at flat offset 64 whose transposed shadow the launch keeps (mst_adam_args.emb)
FORMS = ("plain", "sched", "gnorm", "emb", "emb_sched_gnorm")


def ops():
    from musicstyletransfer_amd import ops as o
    return o


def engine():
    from musicstyletransfer_amd import engine as E
    return E


def test_sizes_cover_what_they_claim():
    """the launch has min(2048, ceil(n / 1024)) workgroups of 256 threads, four elements a thread and round"""
    grid = lambda n: min(2048, max(1, -(-n // 1024)))
    assert [grid(n) for n in SIZES] == [1, 1, 1, 257, 2048]
    assert SIZES[0] // 4 == 0 and SIZES[1] // 4 == 0 and all(n % 4 for n in SIZES)  # every size has a scalar tail
    assert SIZES[3] // 4 <= 257 * 256           # one round: every thread has at most one four-vector
    assert 2048 * 256 < SIZES[4] // 4 < 2 * 2048 * 256  # 256 threads take a second one


# ------------------------------------------------------------------------------------------ kernel level: helpers
def _problem(gpu, n, seed):
    g = torch.Generator().manual_seed(seed)
    p = dict(w=torch.randn(n, generator=g), grad=torch.randn(n, generator=g) * 50, m=torch.randn(n, generator=g) * 0.1,
             v=torch.rand(n, generator=g) * 0.01, ema=torch.randn(n, generator=g), recon=torch.rand(7, generator=g) * 20,
             kl=torch.rand(7, generator=g) * 8)
    p = {k: t.to(gpu) for k, t in p.items()}
    p["sched"] = torch.tensor([0.375, 3.0, 1.0, 6.0], device=gpu)
    return p


def _fresh(gpu, p, dtype, t):
    """the state one launch updates: clones of w, m, v and the average, zeroed shadows, a step state as the step's first launch leaves it"""
    n = p["w"].numel()
    s = dict(w=p["w"].clone(), m=p["m"].clone(), v=p["v"].clone(), ema=p["ema"].clone(), w16=torch.zeros(n, dtype=dtype, device=gpu),
             wt16=torch.zeros(32 * 16, dtype=dtype, device=gpu), total=torch.zeros(7, device=gpu), metric=torch.zeros(3, device=gpu),
             state=torch.tensor([t, 0], dtype=torch.int32, device=gpu), gstat=torch.zeros(8, device=gpu))
    s["state"].view(torch.float32)[1] = LR
    return s


def _launch(o, p, s, form, ema, parts=None, max_norm=1.0, status=None, finite=None):
    """one Adam launch of `form` on state s, in its averaging form (ema=True) or through the existing entry point of that form"""
    emb = dict(base=0, specs=[EMB], wt16=s["wt16"]) if "emb" in form else None
    sched = p["sched"] if "sched" in form else None
    gnorm = dict(parts=parts, max_norm=max_norm, gstat=s["gstat"]) if "gnorm" in form else None
    guard = dict(status=status, expect=[]) if status is not None else {}
    if finite is not None:
        guard["finite"] = finite
    mt = dict(recon=p["recon"], kl=p["kl"], kl_weight=0.5, total=s["total"], metric=s["metric"], **guard)
    kw = dict(ema=dict(buf=s["ema"], decay=DECAY)) if ema else {}
    o.adam_flat(s["w"], p["grad"], s["m"], s["v"], s["w16"], s["state"], lr=LR, rescale=R, clip=0.5, wd=0.01, advance_step=False,
                metrics=mt, emb=emb, sched=sched, gnorm=gnorm, **kw)
    torch.cuda.synchronize()
    return s


KEYS = ("w", "m", "v", "w16", "wt16", "total", "metric", "state", "gstat")


def _same(a, b, what, keys=KEYS):
    for k in keys:
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), (what, k)  # (bytes: a NaN equals itself)


def _parts(o, p, gpu):
    parts = torch.zeros(o.grad_sumsq_parts(), device=gpu)
    o.grad_sumsq(p["grad"], 0, R, R, parts)
    torch.cuda.synchronize()
    return parts, 0.5 * math.sqrt(float(parts.double().sum()))  # a bound at half the norm: the factor is far from any rounding


# ------------------------------------------------------------------------------------------ 1. the averaging form of every form
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_ema_is_the_existing_launch_plus_the_host_rule(gpu, n, dtype):
    E, o = engine(), ops()
    p = _problem(gpu, n, 100 + n % 1000)
    parts, max_norm = _parts(o, p, gpu)
    e0 = p["ema"].cpu().numpy()
    steps = STEPS if n < 2 ** 20 else (1, 890)  # (the largest size is there for the second round, not for the rule)

    def run():
        for form in FORMS:
            for t in steps:
                a = _launch(o, p, _fresh(gpu, p, dtype, t), form, True, parts, max_norm)
                b = _launch(o, p, _fresh(gpu, p, dtype, t), form, False, parts, max_norm)
                _same(a, b, (form, t))
                assert torch.equal(b["ema"], p["ema"]) and int(a["state"][0]) == t
                assert not torch.equal(a["w"], p["w"]) and torch.equal(a["w16"], a["w"].to(dtype))
                d = E.ema_decay_at(t, DECAY)
                want = E.ema_update(e0, a["w"].cpu().numpy(), d)
                got = a["ema"].cpu().numpy()
                assert got.tobytes() == want.tobytes(), (form, t, float(d), int((got != want).sum()), np.abs(got - want).max())
                assert (got != e0).any()
                if "gnorm" in form:
                    assert 0.49 < a["gstat"][1].item() < 0.51  # (clipped: the factor went into the update on both sides)

    names = _calls(o, run)
    # the comparison was, per form, between the launch with the average and the same launch without: the five of FORMS, each as often
    labels = {"plain": "mst_adam_flat", "sched": "mst_adam_flat+sched", "gnorm": "mst_adam_flat+gnorm", "emb": "mst_adam_flat+emb",
              "emb_sched_gnorm": "mst_adam_flat+emb+sched+gnorm"}
    assert [nm for nm in names if nm.startswith("mst_adam_flat")] == [
        labels[form] + tail for form in FORMS for t in steps for tail in ("+ema", "")]
    assert {nm for nm in names if "+ema" not in nm} == {labels[form] for form in FORMS}
    assert sum("+ema" in nm for nm in names) == len(FORMS) * len(steps)
    assert float(E.ema_decay_at(889, DECAY)) < float(E.ema_decay_at(890, DECAY)) == float(np.float32(DECAY))


# ------------------------------------------------------------------------------------------ 2. skipped launches
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", SIZES)
def test_a_skipped_launch_leaves_the_average_alone(gpu, n, dtype):
    """the three guards of the Adam launch, each set as its own tests set it: non-finite norm parts (a NaN in the bucket, which reaches
    the launch only through the parts), a set flag in the sticky status word (a failed position-0 tail), a per-sample loss that is not
    finite. Parameters, moments, shadows and the average keep their bits, the step count is taken back."""
    o = ops()
    p = _problem(gpu, n, 200 + n % 1000)
    T0 = 12
    keys = ("w", "m", "v", "ema", "w16", "wt16", "total", "metric", "gstat")

    def check(s, status, want_status, what):
        ref = _fresh(gpu, p, dtype, T0)
        _same(s, ref, what, keys)
        assert int(s["state"][0]) == T0 - 1 and status.tolist() == want_status, (what, s["state"].tolist(), status.tolist())

    # (a) the norm is not finite
    clean = p["grad"].clone()
    p["grad"][n // 2] = float("nan")
    parts = torch.zeros(o.grad_sumsq_parts(), device=gpu)
    o.grad_sumsq(p["grad"], 0, R, R, parts)
    status = torch.zeros(3, dtype=torch.int32, device=gpu)
    for form in ("gnorm", "emb_sched_gnorm"):
        status.zero_()
        s = _launch(o, p, _fresh(gpu, p, dtype, T0), form, True, parts, 1.0, status=status)
        assert not torch.isfinite(parts).all()
        check(s, status, [0, 0, 1], (form, "norm"))
    p["grad"].copy_(clean)
    # (b) the tail-failure flag; (c) the loss guard
    bad_recon = p["recon"].clone()
    bad_recon[3] = float("inf")
    for form in ("plain", "emb_sched_gnorm"):
        good_parts, max_norm = _parts(o, p, gpu)
        status.zero_()
        status[0] = 1  # MST_TAIL_SPIN_FWD
        s = _launch(o, p, _fresh(gpu, p, dtype, T0), form, True, good_parts, max_norm, status=status)
        check(s, status, [1, 1, 0], (form, "flag"))
        status.zero_()
        s = _launch(o, p, _fresh(gpu, p, dtype, T0), form, True, good_parts, max_norm, status=status, finite=(bad_recon, p["kl"]))
        check(s, status, [0, 0, 1], (form, "loss"))
        # the same launch with nothing wrong counts, and averages
        status.zero_()
        s = _launch(o, p, _fresh(gpu, p, dtype, T0), form, True, good_parts, max_norm, status=status, finite=(p["recon"], p["kl"]))
        assert status.tolist() == [0, 0, 0] and int(s["state"][0]) == T0 and not torch.equal(s["ema"], p["ema"])


# ------------------------------------------------------------------------------------------ 3. the exchange
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", SIZES)
def test_ema_swap_exchanges_exactly_and_twice_is_the_identity(gpu, n, dtype):
    o = ops()
    p = _problem(gpu, n, 300 + n % 1000)
    if n > 8:  # values a swap must not normalise: a NaN payload, infinities, a subnormal, signed zeros
        p["w"][:6] = torch.tensor([float("nan"), float("inf"), -0.0, 1e-41, 65520.0, -3.4e38], device=gpu)
        p["ema"][2:7] = torch.tensor([0.0, float("-inf"), 1e-40, 3.0e38, float("nan")], device=gpu)
    s = _fresh(gpu, p, dtype, 1)
    s["w16"].fill_(7.0)
    w0, e0 = s["w"].cpu().numpy().tobytes(), s["ema"].cpu().numpy().tobytes()
    o.ema_swap(s["w"], s["ema"], s["w16"])
    torch.cuda.synchronize()
    assert s["w"].cpu().numpy().tobytes() == e0 and s["ema"].cpu().numpy().tobytes() == w0
    # w16 is the cast the Adam launch writes: round to nearest even of the new w, which is what the clip tests hold that launch to (on
    # values inside the 16-bit type's normal range; the handful of special values above are there for the exchange)

    def cast_ok():
        w = s["w"]
        plain = torch.isfinite(w) & (w.abs() < 6.0e4) & ((w.abs() > 1e-4) | (w == 0))
        assert plain.sum().item() >= 0.99 * n - 7
        return torch.equal(s["w16"][plain], w.to(dtype)[plain])

    assert cast_ok()
    first = s["w16"].clone()
    o.ema_swap(s["w"], s["ema"], s["w16"])
    torch.cuda.synchronize()
    assert s["w"].cpu().numpy().tobytes() == w0 and s["ema"].cpu().numpy().tobytes() == e0
    assert cast_ok() and not torch.equal(first, s["w16"])


# ------------------------------------------------------------------------------------------ whole steps: helpers
def _small_step(gpu, dtype, seed=13, **hyper):
    """store + plan of the small piano-roll model on a batch of ragged lengths (explicit eps, dropout 0), on the LayerNorm-backward form
    whose sums have a fixed order (LN_PARTIALS_MIN = 0: DESIGN §11, "Where bit-identity is asserted")"""
    from test_step_gpu import _setup
    O, E, ocfg, ecfg, params, batch, eps = _setup("pianoroll", DIMS, B_STEP, T_STEP, seed, ragged=True)
    assert len(set(batch["seq_lens"].tolist())) > 1
    store = E.ParamStore(ecfg, gpu, dtype, params_np=params)
    plan = E.StepPlan(store, B_STEP, T_STEP, clip_gradient=1.0, lr=1e-3, **hyper)
    plan.LN_PARTIALS_MIN = 0
    plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
    return E, store, plan, (ecfg, batch, eps)


def _tensors(store):
    return [t for t in (store.w, store.m, store.v, store.w16, store.wt16, store.step_state, store._metric_buf, store.ema) if t is not None]


def _captured(store, plan, **kw):
    saved = [t.clone() for t in _tensors(store)]
    plan.step_kernels(True)  # (HIP modules load lazily and are not capturable)
    torch.cuda.synchronize()
    plan.capture(True, **kw)
    for t, s in zip(_tensors(store), saved):
        t.copy_(s)


def _calls(o, fn):
    from test_schedule_gpu import _calls as calls
    return calls(o, fn)


def _flat(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    return a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ 4. training untouched, the recurrence, the graph
@pytest.mark.parametrize("extra", [{}, dict(clip_global_norm=0.05, kl_warmup_steps=4, kl_free_bits=2.0, lr_warmup_steps=3)], ids=["alone", "clip+sched"])
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
def test_whole_steps_training_untouched_recurrence_eager_and_nodes(gpu, dtype, extra):
    o = ops()
    E, s_off, p_off, _ = _small_step(gpu, dtype, **extra)
    _, s_zero, p_zero, _ = _small_step(gpu, dtype, ema_decay=0.0, **extra)
    _, s_on, p_on, _ = _small_step(gpu, dtype, ema_decay=DECAY, **extra)
    _, s_eag, p_eag, _ = _small_step(gpu, dtype, ema_decay=DECAY, **extra)
    assert not p_off.forms.ema and not p_zero.forms.ema and p_on.forms.ema and p_on.forms.gnorm == bool(extra) == p_on.forms.sched
    assert s_off.ema is None and s_zero.ema is None and s_on.ema is not None and s_on.ema.data_ptr() != s_on.w.data_ptr()
    assert torch.equal(s_on.ema, s_on.w)  # made as a copy of the weights
    with pytest.raises(RuntimeError, match="average"):
        s_off.to_numpy("ema")
    with pytest.raises(RuntimeError, match="average"):
        s_off.swap_ema()
    two = dtype == F16
    assert (p_on.gscale != p_on.gscale_enc) == two  # fp16: the two-range form
    # (a) off is the old path; on, the same launches in the same order with the Adam launch(es) in the averaging form
    saved = [(s, [t.clone() for t in _tensors(s)]) for s in (s_off, s_zero, s_on)]
    names = {k: _calls(o, lambda: p.step_kernels(True)) for k, p in (("off", p_off), ("zero", p_zero), ("on", p_on))}
    torch.cuda.synchronize()
    adam = [i for i, nm in enumerate(names["off"]) if nm.startswith("mst_adam_flat")]
    assert names["off"] == names["zero"] and not any("+ema" in nm or nm == "mst_ema_swap" for nm in names["off"])
    assert len(adam) == (2 if two else 1) and adam == list(range(adam[0], adam[0] + len(adam)))
    if extra:  # clipped in every range, scheduled where the bookkeeping is: the first
        assert [names["off"][i].replace("+emb", "") for i in adam] == ["mst_adam_flat+sched+gnorm", "mst_adam_flat+gnorm"][: len(adam)]
    else:
        assert {names["off"][i] for i in adam} <= {"mst_adam_flat", "mst_adam_flat+emb"}
    want = list(names["off"])
    for i in adam:
        want[i] = names["off"][i] + "+ema"  # (the same launch otherwise)
    assert names["on"] == want
    assert set(p_off.metrics(reset=False)) == set(p_on.metrics(reset=False))
    for s, was in saved:
        for t, x in zip(_tensors(s), was):
            t.copy_(x)
    # (b) captured: as many nodes, as many kernel launches among them
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
        for s, p in ((s_off, p_off), (s_on, p_on)):
            _captured(s, p)
        assert p_on.graph_nodes() == p_off.graph_nodes() and 0 < p_on.graph_nodes()[1]
        assert torch.equal(s_off.w, s_on.w) and torch.equal(s_on.ema, s_on.w) and int(s_on.step_state[0]) == 0
        # (c) six replays: training bit-identical to the option off, the average the host recurrence over the weights of each step,
        # the captured step the eager one
        e_flat, e_named = _flat(s_on.ema), s_on.to_numpy("ema")
        cut = s_on.offsets["decoder.latent2hid.weight"]
        for t in range(1, 7):
            p_off.run()
            p_on.run()
            p_eag.step_kernels(True)
            torch.cuda.synchronize()
            for k in ("w", "m", "v", "w16", "wt16"):
                assert torch.equal(getattr(s_off, k), getattr(s_on, k)), (t, k)
                assert torch.equal(getattr(s_eag, k), getattr(s_on, k)), (t, k, "eager")
            assert int(s_on.step_state[0]) == int(s_off.step_state[0]) == int(s_eag.step_state[0]) == t
            d = E.ema_decay_at(t, DECAY)
            w_named = s_on.to_numpy("w")
            e_named = {n: E.ema_update(e_named[n], w_named[n], d) for n in e_named}
            got = s_on.to_numpy("ema")
            for n in e_named:
                assert _bits(got[n], e_named[n]), (t, n)
            # the whole bucket, padding words included, with ONE d_t: both ranges of an fp16 step
            e_flat = E.ema_update(e_flat, _flat(s_on.w), d)
            assert _bits(_flat(s_on.ema), e_flat), t
            assert (e_flat[:cut] != _flat(s_on.w)[:cut]).any() and (e_flat[cut:] != _flat(s_on.w)[cut:]).any()
            assert torch.equal(s_eag.ema, s_on.ema), t
        m = p_on.metrics(reset=False)
        assert m["count"] == 6 * B_STEP and m["nonfinite_steps"] == 0 and int(s_on.step_status.cpu()[1]) == 0
        if extra:
            assert m["clip_frac"] > 0  # (the bound was in force: the factor went into both runs alike)


# ------------------------------------------------------------------------------------------ 5. a skipped step
def test_a_step_with_a_nonfinite_gradient_leaves_the_average_and_the_count(gpu):
    """the clip tests' injection: the optimizer in a graph of its own, a stand-in for the all-reduce that writes a NaN into the bucket
    between the graphs; the norm guard of clip_global_norm then skips the step"""
    import warnings
    E, store, plan, _ = _small_step(gpu, BF, ema_decay=DECAY, clip_global_norm=1e6)
    with torch.cuda.stream(torch.cuda.Stream()):
        _captured(store, plan, split_optimizer=True)
        assert plan.graph_opt is not None
        plan.run(reduce_fn=lambda flat: None)
        plan.run(reduce_fn=lambda flat: None)
        torch.cuda.synchronize()
        assert int(store.step_state[0]) == 2 and not torch.equal(store.ema, store.w)
        store.read_metrics(reset=True)
        # (the step state's second word, lr_t, is written by every step's first launch; the count is what a skipped step takes back)
        before = [t.clone() for t in (store.w, store.m, store.v, store.w16, store.ema, store.step_state[:1])]

        def poison(flat):
            flat[flat.numel() // 3] = float("nan")

        plan.run(reduce_fn=poison)
        torch.cuda.synchronize()
        for k, (t, b) in enumerate(zip((store.w, store.m, store.v, store.w16, store.ema, store.step_state[:1]), before)):
            assert torch.equal(t, b), k
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            got = store.read_metrics(reset=True)
        assert got["nonfinite_steps"] == 1 and got["count"] == 0
        plan.run(reduce_fn=lambda flat: None)  # the next clean step is step 3, and averages at d_3
        torch.cuda.synchronize()
        assert int(store.step_state[0]) == 3
        want = E.ema_update(_flat(before[4]), _flat(store.w), E.ema_decay_at(3, DECAY))
        assert _bits(_flat(store.ema), want)


# ------------------------------------------------------------------------------------------ 6. swapped in, swapped out
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "fp16"])
def test_swapped_in_weights_are_a_fresh_stores_and_swap_out_restores_training(gpu, dtype):
    E, s_on, p_on, (ecfg, batch, eps) = _small_step(gpu, dtype, ema_decay=DECAY)
    _, s_twin, p_twin, _ = _small_step(gpu, dtype, ema_decay=DECAY)
    with torch.cuda.stream(torch.cuda.Stream()):
        for s, p in ((s_on, p_on), (s_twin, p_twin)):
            _captured(s, p)
        for _ in range(3):
            p_on.run()
            p_twin.run()
        torch.cuda.synchronize()
        assert torch.equal(s_on.w, s_twin.w) and torch.equal(s_on.ema, s_twin.ema) and not torch.equal(s_on.ema, s_on.w)
        before = [t.clone() for t in _tensors(s_on)]
        ptrs = [t.data_ptr() for t in _tensors(s_on)]
        fresh = E.ParamStore(ecfg, gpu, dtype, params_np=s_on.to_numpy("ema"))

        def infer(store):
            plan = E.StepPlan(store, B_STEP, T_STEP, want_probs=True, internal_eps=False)
            plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
            plan.forward(inference=True)
            plan.losses(with_grad=False, combine=False)
            torch.cuda.synchronize()
            return [t.clone() for t in (plan.mu, plan.sigma, plan.probs)]

        raw = infer(s_on)
        with s_on.ema_weights() as inside:
            assert inside is s_on and s_on.ema_swapped
            torch.cuda.synchronize()
            assert torch.equal(s_on.w, before[7]) and torch.equal(s_on.ema, before[0])  # contents moved ...
            assert [t.data_ptr() for t in _tensors(s_on)] == ptrs                          # ... pointers did not
            a, b = s_on.as_consumed_numpy(), fresh.as_consumed_numpy()
            assert set(a) == set(b) and all(_bits(a[n], b[n]) for n in a)
            assert torch.equal(s_on.w16, fresh.w16) and torch.equal(s_on.wt16, fresh.wt16)
            got, want = infer(s_on), infer(fresh)
            for g, w_, name in zip(got, want, ("mu", "sigma", "probs")):
                assert torch.equal(g, w_), name
            assert not torch.equal(got[0], raw[0])  # (and they are not the raw iterate's)
        torch.cuda.synchronize()
        assert not s_on.ema_swapped
        # (all but wt16: the inference pass and the refresh rebuilt the transposed shadows the next step's first launch rebuilds anyway)
        for k, (t, b) in enumerate(zip(_tensors(s_on), before)):
            assert k == 4 or torch.equal(t, b), k
        # an exception inside swaps back too
        with pytest.raises(KeyError):
            with s_on.ema_weights():
                raise KeyError("inside")
        torch.cuda.synchronize()
        assert not s_on.ema_swapped and torch.equal(s_on.w, before[0]) and torch.equal(s_on.ema, before[7])
        # the graph recorded before the swaps replays on: the next training step is the step of a run that never swapped
        p_on.run()
        p_twin.run()
        torch.cuda.synchronize()
        for k in ("w", "m", "v", "w16", "wt16", "ema"):
            assert torch.equal(getattr(s_on, k), getattr(s_twin, k)), k
        assert int(s_on.step_state[0]) == int(s_twin.step_state[0]) == 4


# ------------------------------------------------------------------------------------------ 7. the trainer
def _model_config():
    from music_style_transfer.VarAutoEncoder import model
    from music_style_transfer.VarAutoEncoder.transformer import TransformerConfig
    P, _, C, Z, De, Le, He, Dd, Ld, Hd = DIMS
    return model.ModelConfig(model.EncoderConfig(TransformerConfig(De, 0.0, Le, He, P), Z, C, P),
                             model.DecoderConfig(TransformerConfig(Dd, 0.0, Ld, Hd, P), Z, C, P), kind="pianoroll")


def _trainer(params, ema_decay):
    """a Trainer on the small piano-roll model, from the weights of _setup (a latent block away from sigma = 0)"""
    from music_style_transfer.VarAutoEncoder import model, trainer
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    cfg = trainer.TrainConfig(batch_size=B_STEP, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                              optimizer=trainer.OptimizerConfig(learning_rate=1e-3, optimizer="adam", optimizer_params="clip_gradient:1.0"),
                              kl_loss=1.0, label_smoothing=0.0, negative_label_downscaling=False, verbose=False, ema_decay=ema_decay)
    t = trainer.Trainer(config=cfg, context=gpu_ctx(0), model=model.Model(_model_config()), sampler=None)
    with torch.cuda.stream(t.stream):
        t.model.store.load_numpy(params)
        if ema_decay > 0:
            t.model.store.load_ema_numpy(None)
    t.stream.synchronize()
    return t


def _steps(t, batch, n):
    for _ in range(n):
        t._step(batch)
        t.train_state.n_batches += 1
    t.stream.synchronize()


SNAP = ("w", "m", "v", "ema", "step_state", "w16", "wt16")


@pytest.fixture(scope="module")
def trained(gpu, tmp_path_factory):
    """three steps with --ema-decay on, a checkpoint with validation; and two steps of a run without it, checkpointed too. Bit-identity
    between trainers is asserted on the fixed-order form of the LayerNorm backward (StepPlan.LN_PARTIALS_MIN = 0), on every side."""
    from test_step_gpu import _setup
    E = engine()
    was = E.StepPlan.LN_PARTIALS_MIN
    E.StepPlan.LN_PARTIALS_MIN = 0
    try:
        O, _, ocfg, ecfg, params, b, eps = _setup("pianoroll", DIMS, B_STEP, T_STEP, 13, ragged=True)
        batch = types.SimpleNamespace(data=[b["x"], b["seq_lens"], b["classes"]], label=[b["labels"]])
        folder = str(tmp_path_factory.mktemp("ema") / "model")
        os.makedirs(folder)
        _model_config().save(os.path.join(folder, "config"))
        t = _trainer(params, DECAY)
        assert t.hyper["ema_decay"] == DECAY and t.model.store.ema is not None
        _steps(t, batch, 3)
        assert t._last_plan.forms.ema
        with torch.cuda.stream(t.stream):
            rng = t._last_plan.rng_state.clone()  # the eps stream as the validation pass finds it
        t.stream.synchronize()
        t._checkpoint(folder, [batch])
        t.stream.synchronize()
        st = t.model.store
        snap = {k: getattr(st, k).clone() for k in SNAP}  # the state the checkpoint holds (a later test steps this trainer on)
        off_folder = str(tmp_path_factory.mktemp("noema") / "model")
        os.makedirs(off_folder)
        _model_config().save(os.path.join(off_folder, "config"))
        t_off = _trainer(params, 0.0)
        assert "ema_decay" not in t_off.hyper and t_off.model.store.ema is None
        _steps(t_off, batch, 2)
        assert not t_off._last_plan.forms.ema
        t_off._checkpoint(off_folder, [batch])
        t_off.stream.synchronize()
        off_snap = {k: getattr(t_off.model.store, k).clone() for k in SNAP if k != "ema"}
        yield dict(E=E, ecfg=ecfg, params=params, batch=batch, folder=folder, t=t, rng=rng, off_folder=off_folder, t_off=t_off, snap=snap,
                   off_snap=off_snap)
    finally:
        E.StepPlan.LN_PARTIALS_MIN = was


def test_checkpoint_files_and_validation_on_the_averaged_weights(gpu, trained):
    E, t, folder, batch, snap = trained["E"], trained["t"], trained["folder"], trained["batch"], trained["snap"]
    st = t.model.store
    named = lambda flat: {n: _flat(flat)[st.offsets[n]: st.offsets[n] + int(np.prod(s))].reshape(s) for n, s in st.shapes.items()}
    # the files: params.N the raw weights, optimizer.N.npz with the average next to the moments; off, no file gains a key
    with np.load(os.path.join(folder, "optimizer.1.npz")) as z:
        assert set(z.files) == {"m", "v", "step_state", "ema"}
        assert _bits(z["ema"], _flat(snap["ema"])) and _bits(z["m"], _flat(snap["m"])) and z["step_state"][0] == 3
    with np.load(os.path.join(folder, "params.1.npz")) as z:
        w = named(snap["w"])
        assert set(z.files) == set(w) and all(_bits(z[n], w[n]) for n in w)
    with np.load(os.path.join(trained["off_folder"], "optimizer.1.npz")) as z:
        assert set(z.files) == {"m", "v", "step_state"}
    assert not torch.equal(snap["ema"], snap["w"]) and not st.ema_swapped  # (swapped back after the validation pass)
    assert set(t.collect_metrics(reset=False)) == set(trained["t_off"].collect_metrics(reset=False))
    # validation ran on the averaged weights: a trainer without the option whose parameters ARE the saved average, handed the same eps
    # stream, reports the same loss. Per-sample losses are fp32 sums of a few atomics in arrival order: equal to a few ulps, 1e-6.
    got = t.last_validation["total_loss"]
    t_avg = _trainer(named(snap["ema"]), 0.0)
    t_raw = _trainer(named(snap["w"]), 0.0)
    losses = []
    for tr in (t_avg, t_raw):
        with torch.cuda.stream(tr.stream):
            tr._plan(B_STEP, T_STEP).rng_state.copy_(trained["rng"])
        tr._step(batch, is_train=False)
        losses.append(tr.collect_metrics(reset=True)["total_loss"])
    print(f"validation total_loss {got!r}; a model of the saved average {losses[0]!r}; of the raw weights {losses[1]!r}")
    assert abs(got - losses[0]) <= 1e-6 * abs(losses[0]) and np.isfinite(got)
    assert abs(got - losses[1]) > 1e-6 * abs(losses[1])  # (and not the raw iterate's)


def test_resume_restores_the_average_and_continues_as_an_uninterrupted_run(gpu, trained, capsys):
    E, t, folder, batch, snap = trained["E"], trained["t"], trained["folder"], trained["batch"], trained["snap"]
    st = t.model.store
    saved = snap["ema"]
    t2 = _trainer(trained["params"], DECAY)
    capsys.readouterr()
    t2._load_latest_checkpoint(folder)
    assert "no averaged weights" not in capsys.readouterr().out
    s2 = t2.model.store
    for k in SNAP:
        assert torch.equal(getattr(s2, k), snap[k]), k
    assert t2.train_state.n_batches == 3 and int(s2.step_state[0]) == 3
    with torch.cuda.stream(t.stream):  # the uninterrupted run, as it stood at the checkpoint
        for k in SNAP:
            getattr(st, k).copy_(snap[k])
    # the eps stream is not part of a checkpoint: hand the uninterrupted run the resumed one's, then one step on each
    with torch.cuda.stream(t2.stream):
        r2 = t2._plan(B_STEP, T_STEP).rng_state.clone()
    t2.stream.synchronize()
    with torch.cuda.stream(t.stream):
        t._last_plan.rng_state.copy_(r2)
    _steps(t, batch, 1)
    _steps(t2, batch, 1)
    for k in ("w", "m", "v", "ema", "step_state"):
        assert torch.equal(getattr(s2, k), getattr(st, k)), k
    assert int(s2.step_state[0]) == 4
    want = E.ema_update(_flat(saved), _flat(s2.w), E.ema_decay_at(4, DECAY))
    assert _bits(_flat(s2.ema), want)


def test_resuming_a_checkpoint_without_the_array_starts_the_average_from_its_weights(gpu, trained, capsys):
    t3 = _trainer(trained["params"], DECAY)
    capsys.readouterr()
    t3._load_latest_checkpoint(trained["off_folder"])
    out = capsys.readouterr().out
    assert out.count("holds no averaged weights") == 1
    s3, off = t3.model.store, trained["off_snap"]
    assert torch.equal(s3.w, off["w"]) and torch.equal(s3.ema, s3.w) and torch.equal(s3.m, off["m"]) and int(s3.step_state[0]) == 2
    # a run without the option reads a checkpoint that has the array as it always did
    t4 = _trainer(trained["params"], 0.0)
    t4._load_latest_checkpoint(trained["folder"])
    assert t4.model.store.ema is None and torch.equal(t4.model.store.w, trained["snap"]["w"]) and int(t4.model.store.step_state[0]) == 3


def test_generate_ema_decodes_with_the_averaged_weights(gpu, trained, tmp_path):
    from music_style_transfer.VarAutoEncoder import sampler as S
    from music_style_transfer.VarAutoEncoder.utils import gpu as gpu_ctx
    from musicstyletransfer_amd import generate as G
    t, folder = trained["t"], trained["folder"]
    st = t.model.store
    # a checkpoint whose params ARE the average
    twin = str(tmp_path / "twin")
    os.makedirs(twin)
    _model_config().save(os.path.join(twin, "config"))
    with np.load(os.path.join(folder, "optimizer.1.npz")) as z:
        ema_flat = z["ema"].copy()
    named = {n: ema_flat[st.offsets[n]: st.offsets[n] + int(np.prod(s))].reshape(s) for n, s in st.shapes.items()}
    np.savez(os.path.join(twin, "params.1.npz"), **named)
    m_ema = S.load_inference_model(folder, gpu_ctx(0), -1, ema=True)
    m_twin = S.load_inference_model(twin, gpu_ctx(0), -1)
    m_raw = S.load_inference_model(folder, gpu_ctx(0), -1)
    torch.cuda.synchronize()
    a, b, c = m_ema.store.as_consumed_numpy(), m_twin.store.as_consumed_numpy(), m_raw.store.as_consumed_numpy()
    assert all(_bits(a[n], b[n]) for n in a) and torch.equal(m_ema.store.wt16, m_twin.store.wt16)
    assert any(not _bits(a[n], c[n]) for n in a) and torch.equal(m_raw.store.w, trained["snap"]["w"])
    assert torch.equal(m_ema.store.w, trained["snap"]["ema"])
    flags = ["--checkpoint", "-1", "--mode", "prior", "--n", "3", "--length", "6", "--decoder", "sampling", "--seed", "1"]
    f_ema = G.main(["--model-output", folder, "--out", str(tmp_path / "a"), "--ema"] + flags)
    f_twin = G.main(["--model-output", twin, "--out", str(tmp_path / "b")] + flags)
    assert len(f_ema) == 3 and [os.path.basename(f) for f in f_ema] == [os.path.basename(f) for f in f_twin]
    for x, y in zip(f_ema, f_twin):
        assert open(x, "rb").read() == open(y, "rb").read() and os.path.getsize(x) > 0
    # without such an array: a clear error, no traceback of a missing key
    with pytest.raises(SystemExit, match="no averaged weights"):
        G.main(["--model-output", trained["off_folder"], "--out", str(tmp_path / "c"), "--ema"] + flags)
    with pytest.raises(SystemExit, match="no averaged weights"):
        G.main(["--model-output", twin, "--out", str(tmp_path / "d"), "--ema"] + flags)  # (no optimizer file at all)
    with pytest.raises(ValueError, match="no averaged weights"):
        S.load_inference_model(trained["off_folder"], gpu_ctx(0), -1, ema=True)
