"""Per-dimension latent statistics on a real MI355X: mst_latent_dim_stats against the sequential fp64 loop of
tests/latent_stats_refs.py (planes 0-3 bit for bit, plane 4 to an ulp of the logarithm per term), the launch inside whole captured
steps (weights untouched, one kernel node more, the sums of three steps, reset, inference), and the trainer's five scalars."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_stats_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = -7.25          # what the cells in front of and behind the accumulator hold
KL_RTOL = 1e-12        # plane 4: |got - ref| <= KL_RTOL * sum |kl_d| of the cell — B <= 512 terms of at most four fp64 roundings
                       # each (2^-53), where the device's log and numpy's may differ by an ulp
SCALARS = ("active_units", "kl_dims_used", "kl_dim_max", "sigma_rms", "class_leak")


class Acc:
    """the [C, 5, Z] fp64 accumulator, zeroed, between two guard stretches of one allocation"""

    def __init__(self, gpu, C, Z):
        n = C * 5 * Z
        self.flat = torch.full((16 + n + 16,), GUARD, dtype=torch.float64, device=gpu)
        self.t = self.flat[16:16 + n].view(C, 5, Z)
        self.t.zero_()

    def read(self):
        h = self.flat.cpu().numpy()
        assert (h[:16] == GUARD).all() and (h[-16:] == GUARD).all(), "a store in front of or behind the accumulator"
        return h[16:-16].reshape(self.t.shape).copy()


def _dev(gpu, mu, sg, cl):
    return torch.from_numpy(mu).to(gpu), torch.from_numpy(sg).to(gpu), torch.from_numpy(cl).to(gpu)


def _check(got, mu, sg, cl, C, ref=None, what=""):
    """planes 0-3 equal to the reference in every bit, plane 4 within KL_RTOL of the cell's sum of |kl_d|; prints the largest
    plane-4 distance in units of that bound first"""
    ref = R.dim_stats_ref(mu, sg, cl, C) if ref is None else ref
    tol = KL_RTOL * R.abs_kl_sums(mu, sg, cl, C)
    d = np.abs(got[:, 4] - ref[:, 4])
    worst = float((d / np.where(tol > 0, tol, 1.0)).max())
    print(f"\n{what}: counted {int(ref[:, 0].sum())} terms; plane 4 worst |got - ref| / bound = {worst:.3g}")
    assert np.isfinite(got).all()
    assert got[:, :4].tobytes() == ref[:, :4].tobytes(), f"{what}: planes 0-3 differ from the sequential fp64 sums"
    assert (d <= tol).all(), f"{what}: plane 4 off by {worst} bounds"


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("Z", [1, 64, 65, 256])
@pytest.mark.parametrize("B", [1, 5, 64, 67])
def test_kernel_against_the_sequential_fp64_loop(gpu, B, Z, C):
    """padded rows whose pad columns hold NaN; a negative sigma, sigma == 0 (+0 and -0), a NaN mu, an inf sigma, classes -1 and C
    planted (B >= 5 for the classes). C = 5 takes two class passes, Z = 65 and 256 more than one workgroup, B = 5 and 67 a ragged
    last chunk of rows."""
    from musicstyletransfer_amd import ops as o
    mu, sg, cl = R.planted(np.random.default_rng(B * 100000 + Z * 100 + C), B, Z, C)
    dmu, dsg, dcl = _dev(gpu, mu, sg, cl)
    acc = Acc(gpu, C, Z)
    o.latent_dim_stats(dmu[:, :Z], dsg[:, :Z], dcl, acc.t)
    torch.cuda.synchronize()
    _check(acc.read(), mu[:, :Z], sg[:, :Z], cl, C, what=f"B {B} Z {Z} C {C}")


def test_a_second_launch_adds(gpu):
    """two batches into one accumulator: the counts are those of the concatenated batch; planes 1-4 are the first launch's sums
    plus the second's (one more rounded addition per cell, bit for bit in planes 1-3), which lies within the distance of two
    summation orders of the concatenated batch's terms"""
    from musicstyletransfer_amd import ops as o
    B1, B2, Z, C = 67, 5, 65, 5
    rng = np.random.default_rng(77)
    a, b = R.planted(rng, B1, Z, C), R.planted(rng, B2, Z, C)
    acc = Acc(gpu, C, Z)
    for mu, sg, cl in (a, b):
        dmu, dsg, dcl = _dev(gpu, mu, sg, cl)
        o.latent_dim_stats(dmu[:, :Z], dsg[:, :Z], dcl, acc.t)
    torch.cuda.synchronize()
    got = acc.read()
    ra, rb = (R.dim_stats_ref(mu[:, :Z], sg[:, :Z], cl, C) for mu, sg, cl in (a, b))
    mu, sg, cl = (np.concatenate([x, y])[:, :Z] if x.ndim == 2 else np.concatenate([x, y]) for x, y in zip(a, b))
    whole = R.dim_stats_ref(mu, sg, cl, C)
    assert np.array_equal(got[:, 0], whole[:, 0]) and whole[:, 0].sum() > B1 * Z
    _check(got, mu, sg, cl, C, ref=ra + rb, what="two launches against the sum of two references")
    tol = KL_RTOL * R.abs_sums(mu, sg, cl, C)  # (far above 2 (B1 + B2) 2^-53 sum |term|, the distance of two orders)
    assert (np.abs(got - whole) <= tol).all(), float((np.abs(got - whole) / np.where(tol > 0, tol, 1)).max())


def test_a_launch_is_reproducible(gpu):
    from musicstyletransfer_amd import ops as o
    mu, sg, cl = R.planted(np.random.default_rng(3), 64, 256, 5)
    dmu, dsg, dcl = _dev(gpu, mu, sg, cl)
    runs = []
    for _ in range(2):
        acc = Acc(gpu, 5, 256)
        o.latent_dim_stats(dmu[:, :256], dsg[:, :256], dcl, acc.t)
        torch.cuda.synchronize()
        runs.append(acc.read().tobytes())
    assert runs[0] == runs[1]


def test_bad_arguments_return_a_status(gpu):
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    mu = torch.zeros(4, 8, device=gpu)
    cl = torch.zeros(4, dtype=torch.int32, device=gpu)
    acc = Acc(gpu, 2, 8)
    good = [4, 8, 2, mu.data_ptr(), 8, mu.data_ptr(), 8, cl.data_ptr(), acc.t.data_ptr(), None]
    for i, bad in ((0, 0), (1, 0), (2, 0), (1, -8), (3, None), (4, 7), (5, None), (6, 7), (7, None), (8, None)):
        args = list(good)
        args[i] = bad
        rc = lib.mst_latent_dim_stats(*args)
        assert rc != 0 and b"mst_latent_dim_stats" in lib.mst_last_error(), (i, bad)
    with pytest.raises(_lib.MstError):
        _lib.call("mst_latent_dim_stats", 4, 8, 2, mu.data_ptr(), 4, mu.data_ptr(), 8, cl.data_ptr(), acc.t.data_ptr(), None)
    torch.cuda.synchronize()
    assert not acc.read().any()  # nothing was launched


# ------------------------------------------------------------------------------------------ whole steps
DIMS = (128, 128, 3, 32, 64, 1, 4, 64, 2, 4)  # the small piano-roll model of tests/test_schedule_gpu.py / test_clip_gpu.py
B_STEP, T_STEP, STEPS = 4, 33, 3


def _small_step(gpu, track):
    from test_step_gpu import _setup
    O, E, ocfg, ecfg, params, batch, eps = _setup("pianoroll", DIMS, B_STEP, T_STEP, 13, ragged=False)
    store = E.ParamStore(ecfg, gpu, torch.bfloat16, params_np=params)
    plan = E.StepPlan(store, B_STEP, T_STEP, clip_gradient=1.0, lr=1e-3)
    plan.LN_PARTIALS_MIN = 0  # the order-free LayerNorm-backward form, on both sides (tests/test_schedule_gpu.py: _order_free)
    plan.track_latent_stats = track
    plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
    return E, store, plan, batch


def _names(o, fn):
    names, real = [], o.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)

    o.call = call
    try:
        fn()
    finally:
        o.call = real
    return names


def _kl_bound(mu, sg):
    """what the latent launch's fp32 kl [B] is held to against the fp64 sum of its terms (tests/latent_refs.py: fwd_refs, 'kl'),
    per sample"""
    from latent_refs import U
    m, s = mu.astype(np.float64), sg.astype(np.float64)
    s2 = s * s
    L = np.log(s2)
    term = 0.5 * (s2 + m * m - 1 - L)
    A = s2 + m * m + 1 + np.abs(L)
    ulp_log = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(L), 2.0 ** -126))) - 23)
    terr = 0.5 * (4 * U * A + U + 2 * ulp_log)
    return terr.sum(1) + mu.shape[1] * U * (np.abs(term) + terr).sum(1)


def test_three_captured_steps_with_the_flag_on_and_off(gpu):
    from musicstyletransfer_amd import ops as o
    from latent_refs import U
    Z, C = DIMS[3], DIMS[2]
    out = {}
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the legacy default stream cannot be captured)
        for track in (False, True):
            E, store, plan, batch = _small_step(gpu, track)
            saved = [t.clone() for t in (store.w, store.m, store.v, store.w16, store.wt16, store.step_state, store._metric_buf)]
            names = _names(o, lambda: plan.step_kernels(True))  # (eager first: HIP modules load lazily and are not capturable)
            torch.cuda.synchronize()
            nodes = plan.capture(True).graph_nodes()
            for t, s in zip((store.w, store.m, store.v, store.w16, store.wt16, store.step_state, store._metric_buf), saved):
                t.copy_(s)
            store.read_metrics(reset=True)
            assert not store.lat_stats.any()
            seen = []
            for _ in range(STEPS):
                plan.run()
                torch.cuda.synchronize()
                seen.append((plan.mu.cpu().numpy().copy(), plan.sigma.cpu().numpy().copy()))
            out[track] = dict(E=E, store=store, plan=plan, names=names, nodes=nodes, seen=seen, w=store.w.clone(), m=store.m.clone(),
                              v=store.v.clone(), classes=batch["classes"].numpy().astype(np.int32))
        off, on = out[False], out[True]
        # off is the old path; on adds one entry point directly behind the latent block's, and one kernel node
        assert "mst_latent_dim_stats" not in off["names"]
        i = on["names"].index("mst_latent_dim_stats")
        assert on["names"][i - 1].startswith("mst_latent_fwd") and on["names"][:i] + on["names"][i + 1:] == off["names"]
        assert on["nodes"] == (off["nodes"][0] + 1, off["nodes"][1] + 1), (off["nodes"], on["nodes"])
        # the launch writes nothing but the accumulator: same weights and moments, bit for bit, and the same posterior in every step
        for k in ("w", "m", "v"):
            assert torch.equal(off[k], on[k]), k
        for (m0, s0), (m1, s1) in zip(off["seen"], on["seen"]):
            assert m0.tobytes() == m1.tobytes() and s0.tobytes() == s1.tobytes()
        assert not off["store"].lat_stats.any()
        # the accumulator: the three steps' references, added in step order
        store, plan, cl = on["store"], on["plan"], on["classes"]
        metrics = store.read_metrics(reset=False)
        got = metrics["lat_stats"]
        assert got.dtype == np.float64 and got.shape == (C, 5, Z)
        ref, tol = np.zeros((C, 5, Z)), np.zeros((C, Z))
        for mu, sg in on["seen"]:
            ref = ref + R.dim_stats_ref(mu, sg, cl, C)
            tol += KL_RTOL * R.abs_kl_sums(mu, sg, cl, C)
        assert got[:, 0].sum() == STEPS * B_STEP * Z and got[:, :4].tobytes() == ref[:, :4].tobytes()
        d = np.abs(got[:, 4] - ref[:, 4])
        print(f"\nthree steps: plane 4 worst |got - ref| / bound = {float((d / tol.clip(1e-300)).max()):.3g}")
        assert (d <= tol).all()
        # ... and its KL agrees with the mean the step itself logs: fp32 per-sample sums (the latent launch's bound per sample,
        # tests/latent_refs.py) added up in fp32 by the step's bookkeeping (N terms in any order: (N - 1) u of their absolute sum)
        N = STEPS * B_STEP
        assert metrics["count"] == N
        kl_mean = got[:, 4].sum() / N
        kl_b = np.concatenate([R.kl_terms(mu, sg).sum(1) for mu, sg in on["seen"]])
        bound = (sum(_kl_bound(mu, sg).sum() for mu, sg in on["seen"]) + N * U * np.abs(kl_b).sum()) / N
        print(f"kl per sample: {kl_mean!r} from the accumulator, {metrics['kl_sum'] / N!r} logged, bound {bound:.3g}")
        assert abs(kl_mean - metrics["kl_sum"] / metrics["count"]) <= bound
        scores = on["E"].latent_scores(got)
        assert abs(scores["kl_dims"].sum() - kl_mean) <= 1e-12 * kl_mean and 0 <= scores["active_units"] <= Z
        # reset clears it; an inference pass leaves it alone; a validation step counts
        assert store.read_metrics(reset=True)["lat_stats"].tobytes() == got.tobytes()
        assert not store.read_metrics(reset=False)["lat_stats"].any()
        plan.forward(inference=True)
        plan.forward(inference=True, upto="latent")
        torch.cuda.synchronize()
        assert not store.lat_stats.any()
        plan.step_kernels(False)
        torch.cuda.synchronize()
        val = store.read_metrics(reset=True)["lat_stats"]
        want = R.dim_stats_ref(plan.mu.cpu().numpy(), plan.sigma.cpu().numpy(), cl, C)
        assert val[:, :4].tobytes() == want[:, :4].tobytes() and val[:, 0].sum() == B_STEP * Z
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ trainer level
def test_trainer_reports_the_five_scalars(gpu, tmp_path, monkeypatch):
    from music_style_transfer.VarAutoEncoder import main
    from music_style_transfer.VarAutoEncoder.data import ToyData
    import json
    logdir = tmp_path / "tb"
    monkeypatch.setenv("MST_LOGDIR", str(logdir))
    folder = str(tmp_path / "toy")
    t = main.main(["--toy", "--gpu", "--max-steps", "3", "--latent-stats", "--model-output", folder])
    assert t.config.latent_stats is True and t._last_plan.track_latent_stats
    Z = t._last_plan.cfg.latent_dim
    got = t.collect_metrics(reset=False)
    print(f"\ntoy, three steps: { {k: got[k] for k in SCALARS} }")

    def sane(m):
        assert set(SCALARS) <= set(m)
        assert isinstance(m["active_units"], int) and 0 <= m["active_units"] <= Z
        assert isinstance(m["kl_dims_used"], int) and 0 <= m["kl_dims_used"] <= Z
        assert math.isnan(m["class_leak"]) or 0.0 <= m["class_leak"] <= 1.0
        assert m["kl_dim_max"] >= 0 and m["sigma_rms"] > 0

    sane(got)
    full = t.last_latent_stats
    assert full["kl_dims"].shape == (Z,) and full["kl_dim_max"] == got["kl_dim_max"] == float(full["kl_dims"].max())
    # three steps of three samples, one of each class, in every dimension
    with torch.cuda.stream(t.stream):
        acc = t.model.store.read_metrics(reset=False)["lat_stats"]
    assert acc.shape == (3, 5, Z) and (acc[:, 0] == 3).all()
    assert abs(full["kl_dims"].sum() - got["kl_loss"]) <= 1e-3 * got["kl_loss"]  # (the logged mean is an fp32 sum of fp32 sums)
    # the validation pass of a checkpoint reports them over the validation set alone, and the scalar log carries them
    t._checkpoint(os.path.join(folder, "model"), ToyData())
    sane(t.last_validation)
    assert "total_loss" in t.last_validation
    with torch.cuda.stream(t.stream):
        assert not t.model.store.read_metrics(reset=False)["lat_stats"].any()  # (read and reset by the validation's collect)
    t._step(next(iter(ToyData())))
    t._periodic_log(0, 0.0)
    tags = {json.loads(line)["tag"] for line in open(logdir / "scalars.jsonl")}
    assert set(SCALARS) <= tags


def test_without_the_flag_none_of_the_keys_appear(gpu, tmp_path, monkeypatch):
    from music_style_transfer.VarAutoEncoder import main
    monkeypatch.setenv("MST_LOGDIR", str(tmp_path / "tb"))
    t = main.main(["--toy", "--gpu", "--max-steps", "2", "--model-output", str(tmp_path / "toy")])
    assert t.config.latent_stats is False and not t._last_plan.track_latent_stats and t.last_latent_stats is None
    got = t.collect_metrics(reset=False)
    assert not set(SCALARS) & set(got) and "kl_loss" in got
    t._checkpoint(str(tmp_path / "toy" / "model"), None)
    with torch.cuda.stream(t.stream):
        assert not t.model.store.lat_stats.any()
