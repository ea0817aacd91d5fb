"""The importance-weighted bound without a GPU: the fp64 reference of the device arithmetic (tests/iw_refs.py) against a two-pass
logsumexp, deliberate mistakes in that reference against the bounds the GPU test uses, the argument checks of mst_iw_fold /
mst_iw_finish (which run before any HIP call), and the host-side pieces: engine.check_iw, engine.iw_scores, the flags."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iw_refs as R  # noqa: E402


def _fold_all(lws):
    """lws [K, B] -> (state, out, acc) through the recurrence"""
    st = np.zeros((lws.shape[1], 6))
    for lw in lws:
        st = R.fold_lw(st, lw)
    out, acc = R.finish(st)
    return st, out, acc


def _lw_sets():
    rng = np.random.default_rng(20271)
    far = np.arange(6)[:, None] * 1000.0 + rng.standard_normal((6, 3))
    return {"random": rng.standard_normal((16, 5)) * 3.0 - 700.0, "random-wide": rng.standard_normal((9, 4)) * 60.0,
            "ascending-1000": far, "descending-1000": far[::-1].copy(), "one-draw": rng.standard_normal((1, 7)) * 5.0 - 4000.0}


@pytest.mark.parametrize("name", list(_lw_sets()))
def test_the_recurrence_is_the_two_pass_logsumexp(name):
    lws = _lw_sets()[name]
    K, B = lws.shape
    st, out, acc = _fold_all(lws)
    for b in range(B):
        log_px, elbo, ess = R.logsumexp_bound(lws[:, b])
        tol = 1e-12 * (1.0 + np.abs(lws[:, b]).sum())
        assert abs(out[b, 0] - log_px) <= tol and abs(out[b, 1] - elbo) <= tol and abs(out[b, 2] - ess) <= 1e-12 * ess
        assert st[b, R.M] == lws[:, b].max() and out[b, 3] == K == st[b, R.N] and st[b, R.N_BAD] == 0
        # Jensen, and the range of the effective sample size (up to the rounding of the sums)
        assert out[b, 0] - out[b, 1] >= -tol, "iw_gap >= 0"
        assert 1.0 - 1e-12 <= out[b, 2] <= K + 1e-12
        if K == 1:
            assert out[b, 0] == out[b, 1] == lws[0, b] and out[b, 2] == 1.0
    assert acc[4] == B and acc[5] == 0 and acc[3] == K * B
    np.testing.assert_allclose(acc[:3], out[:, :3].sum(0), rtol=1e-14)


def test_a_bad_draw_enters_n_bad_only_and_finish_adds():
    lws = np.array([[1.0, 2.0, 3.0], [np.nan, 2.5, -np.inf], [0.5, np.inf, 3.5]])
    st, out, acc = _fold_all(lws)
    assert st[:, R.N].tolist() == [2, 2, 2] and st[:, R.N_BAD].tolist() == [1, 1, 1]
    assert np.isnan(out[:, :3]).all() and out[:, 3].tolist() == [2, 2, 2] and acc.tolist() == [0, 0, 0, 0, 0, 3]
    st2, out2, _ = _fold_all(lws[[0, 2]][:, [0, 2]])  # (the finite draws of samples 0 and 2 alone)
    assert np.array_equal(st[[0, 2], :5], st2[:, :5])
    # an empty state is invalid too; acc is added to
    out3, acc3 = R.finish(np.zeros((2, 6)), acc=np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))
    assert np.isnan(out3[:, :3]).all() and (out3[:, 3] == 0).all() and acc3.tolist() == [1, 2, 3, 4, 5, 8]


@pytest.mark.parametrize("B,Z", R.KERNEL_SHAPES)
@pytest.mark.parametrize("draws", R.KERNEL_DRAWS)
def test_mutants_leave_the_bounds_of_the_gpu_test(B, Z, draws):
    """the kernel-level comparison (iw_refs.compare) accepts the reference itself and sees each deliberate mistake"""
    case = R.kernel_case(B, Z, draws)
    st, mag = R.fold_case(case)
    out, _ = R.finish(st)
    assert R.compare(st, out, st, out, mag) == []
    specials = R.special_rows(B)
    for b, what in specials.items():  # the special samples are what they claim to be
        if what in ("sigma0", "nan_eps", "inf_recon"):
            assert st[b, R.N_BAD] == 1 and st[b, R.N] == draws - 1 and np.isnan(out[b, 0])
        elif draws > 1:
            lw = np.array([R.log_weight(case["eps"][k], case["sigma"][k], case["z"][k], case["recon"][k], case["recon_scale"])[0][b]
                           for k in range(draws)])
            step = np.diff(lw)
            assert (step > 700).all() if what == "asc800" else (step < -700).all()
    assert all(st[b, R.N_BAD] == 0 and st[b, R.N] == draws for b in range(B) if b not in specials or specials[b].endswith("800"))
    for mutant in R.MUTANTS:
        # (with one draw log n = 0 and nothing is ever rescaled: those two mistakes cannot show there; a rescale needs a rising weight)
        if mutant == "no_log_n" and draws == 1:
            continue
        if mutant == "no_s2_rescale" and (draws == 1 or B < 2):
            continue
        mst, _ = R.fold_case(case, mutant)
        mout, _ = R.finish(mst, mutant=mutant)
        assert R.compare(mst, mout, st, out, mag), f"{mutant} stays within the bounds at B {B} Z {Z} draws {draws}"


# --------------------------------------------------------------------------------------------------- the two entry points
@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _host_block(n_bytes=4096):
    """an address that is never followed: the checks under test refuse the call before any HIP call"""
    buf = ctypes.create_string_buffer(n_bytes + 64)
    addr = (ctypes.addressof(buf) + 63) // 64 * 64
    return buf, addr


def test_abi_122_declares_and_exports_both(lib):
    from musicstyletransfer_amd import _lib
    i64, f64, vp, ci = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_int
    assert lib.mst_version() >= 122
    assert _lib.SIGNATURES["mst_iw_fold"] == (ci, [i64, i64, vp, i64, vp, i64, vp, i64, vp, f64, vp, vp])
    assert _lib.SIGNATURES["mst_iw_finish"] == (ci, [i64, vp, vp, vp, vp])
    assert hasattr(lib, "mst_iw_fold") and hasattr(lib, "mst_iw_finish")


FOLD_OK = dict(B=4, Z=8, eps=1, ld_eps=8, sigma=1, ld_sigma=8, z=1, ld_z=8, recon=1, recon_scale=64.0, state=1)
FOLD_BAD = [
    (dict(eps=0), b"null pointer"), (dict(sigma=0), b"null pointer"), (dict(z=0), b"null pointer"), (dict(recon=0), b"null pointer"),
    (dict(state=0), b"null pointer"),
    (dict(B=0), b"B and Z must be positive"), (dict(B=-3), b"B and Z must be positive"), (dict(Z=0), b"B and Z must be positive"),
    (dict(ld_eps=7), b"< Z"), (dict(ld_sigma=7), b"< Z"), (dict(ld_z=0), b"< Z"),
    (dict(state=8), b"state must be 16-byte aligned"),
    (dict(recon_scale=0.0), b"recon_scale must be finite and > 0"), (dict(recon_scale=-2.0), b"recon_scale must be finite and > 0"),
    (dict(recon_scale=float("inf")), b"recon_scale must be finite and > 0"), (dict(recon_scale=float("nan")), b"recon_scale must be finite and > 0"),
]


@pytest.mark.parametrize("change,message", FOLD_BAD, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in FOLD_BAD])
def test_iw_fold_refuses_before_any_hip_call(lib, change, message):
    keep, base = _host_block()
    a = dict(FOLD_OK, **change)
    p = lambda v: None if v == 0 else base + (v - 1)  # 0: NULL, 1: the aligned block, 8: eight bytes behind it
    rc = lib.mst_iw_fold(a["B"], a["Z"], p(a["eps"]), a["ld_eps"], p(a["sigma"]), a["ld_sigma"], p(a["z"]), a["ld_z"], p(a["recon"]),
                         a["recon_scale"], None if a["state"] == 0 else base + (0 if a["state"] == 1 else a["state"]), None)
    assert rc == -1 and message in lib.mst_last_error(), lib.mst_last_error()


FINISH_BAD = [(dict(state=0), b"null pointer"), (dict(out=0), b"null pointer"), (dict(acc=0), b"null pointer"),
              (dict(B=0), b"B must be positive"), (dict(state=8), b"state must be 16-byte aligned"),
              (dict(out=4), b"8-byte aligned"), (dict(acc=4), b"8-byte aligned")]


@pytest.mark.parametrize("change,message", FINISH_BAD, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in FINISH_BAD])
def test_iw_finish_refuses_before_any_hip_call(lib, change, message):
    keep, base = _host_block()
    a = dict(dict(B=4, state=1, out=1, acc=1), **change)
    p = lambda v, off: None if v == 0 else base + off + (0 if v == 1 else v)
    rc = lib.mst_iw_finish(a["B"], p(a["state"], 0), p(a["out"], 1024), p(a["acc"], 2048), None)
    assert rc == -1 and message in lib.mst_last_error(), lib.mst_last_error()


# --------------------------------------------------------------------------------------------------- host side
def test_check_iw():
    from musicstyletransfer_amd import engine as E
    for ok in (1, 2, 64, np.int64(5), 10 ** 6):
        E.check_iw(ok)
    for bad in (0, -1, 1.5, 2.0, float("nan"), float("inf"), None, "4", True):
        with pytest.raises(ValueError, match="iw_samples"):
            E.check_iw(bad)


def test_train_config_and_flags():
    from music_style_transfer.VarAutoEncoder import config, generate as G, main, trainer
    assert config.get_config([]).iw_samples == 0 and config.get_config(["--iw-samples", "8"]).iw_samples == 8
    assert main.create_toy_train_config(iw_samples=4).iw_samples == 4 and main.create_toy_train_config().iw_samples == 0
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="iw_samples"):
            main.create_toy_train_config(iw_samples=bad)
    assert "iw_samples" in trainer.TrainConfig.__init__.__code__.co_varnames
    assert "likelihood" in G.MODES
    a = G.build_parser().parse_args(["--model-output", "m", "--mode", "likelihood", "--toy", "--iw-samples", "5"])
    assert (a.mode, a.iw_samples, a.out) == ("likelihood", 5, None)
    for script in ("train-vae.sh", "generate-vae.sh"):
        assert "--iw-samples" in open(os.path.join(ROOT, "scripts", script)).read()


def test_iw_scores():
    from musicstyletransfer_amd import engine as E
    acc = np.array([-300.0, -330.0, 7.5, 12.0, 3.0, 1.0])
    s = E.iw_scores(acc, cells=64)
    assert s["iw_nll"] == 100.0 and s["iw_elbo_nll"] == 110.0 and s["iw_gap"] == 10.0 and s["iw_ess"] == 2.5 and s["iw_invalid"] == 1
    assert s["iw_bits_per_cell"] == 100.0 / (64 * math.log(2.0))
    assert set(s) == {"iw_nll", "iw_elbo_nll", "iw_gap", "iw_ess", "iw_bits_per_cell", "iw_invalid"}
    empty = E.iw_scores(np.array([0.0, 0, 0, 0, 0, 2]), cells=16)
    assert math.isnan(empty["iw_nll"]) and math.isnan(empty["iw_gap"]) and math.isnan(empty["iw_ess"]) and empty["iw_invalid"] == 2
    # from the reference's own sums: the gap is Jensen's, the figures are per piece
    lws = np.random.default_rng(5).standard_normal((8, 6)) * 4.0 - 50.0
    _, out, racc = _fold_all(lws)
    s = E.iw_scores(racc, cells=10)
    assert s["iw_gap"] >= 0 and abs(s["iw_nll"] + out[:, 0].mean()) <= 1e-12 and 1.0 <= s["iw_ess"] <= 8.0
    with pytest.raises(ValueError):
        E.iw_scores(np.zeros(5), cells=4)
    with pytest.raises(ValueError):
        E.iw_scores(acc, cells=0)


ENGINE_CASES = {  # the engine-level GPU cases (tests/test_iw_gpu.py): kind, dims, B, T, seed
    "roll-d128": ("pianoroll", (128, 128, 2, 32, 64, 2, 4, 128, 1, 4), 4, 64, 301),
    "roll-d64": ("pianoroll", (128, 128, 3, 32, 64, 1, 4, 64, 2, 4), 4, 64, 302),
    "token": ("token", (10, 10, 3, 16, 32, 1, 2, 32, 1, 2), 4, 16, 303),
}


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_the_oracle_leaves_no_sample_invalid_at_the_gpu_tests_seeds(name):
    """the engine-level GPU test compares with the oracle at the draws the device recorded; here the same models and batches go through
    the oracle on the CPU at stand-in draws: sigma stays away from 0 (it does not depend on the draw) and every log-weight is finite"""
    import torch
    from test_step_gpu import _setup
    kind, dims, B, T, seed = ENGINE_CASES[name]
    O, E, ocfg, ecfg, params, batch, eps = _setup(kind, dims, B, T, seed)
    P = O.to_torch_params(params, requires_grad=False)
    rng = np.random.default_rng(seed)
    cells = T * (dims[1] if kind == "pianoroll" else 1)
    st = np.zeros((B, 6))
    for _ in range(4):
        e = torch.from_numpy(rng.standard_normal((B, dims[3])).astype(np.float32))
        with torch.no_grad():
            _, recon, _, _, means, stds = O.step_losses(P, ocfg, batch, e)
        assert float(stds.abs().min()) > 0.2
        st = R.fold(st, e.numpy(), stds.numpy(), (means + e * stds).numpy(), recon.numpy(), float(cells))
    out, acc = R.finish(st)
    assert acc[4] == B and acc[5] == 0 and np.isfinite(out).all()
    assert (out[:, 0] - out[:, 1] >= 0).all() and (out[:, 2] >= 1 - 1e-12).all() and (out[:, 2] <= 4 + 1e-12).all()
