"""The class-conditional MMD penalty without a GPU: the fp64 reference of tests/class_mmd_refs.py against torch autograd of the
per-class definition, the linear-kernel identity with the between-class variance, the degenerate cases, class_mmd_score, the flags and
TrainConfig, the header's declaration and the argument checks of mst_class_mmd (which come before any HIP call)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_mmd_refs as R  # noqa: E402

SHAPES = [(4, 32, 3), (64, 64, 2), (5, 65, 5), (67, 256, 5), (1, 8, 1), (2, 1, 2)]  # (B, Z, C)


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _train_config(**kw):
    from musicstyletransfer_amd.VarAutoEncoder import trainer
    return trainer.TrainConfig(batch_size=8, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                               optimizer=trainer.OptimizerConfig(learning_rate=3e-4, optimizer="adam", optimizer_params="clip_gradient:1.0"),
                               kl_loss=0.5, label_smoothing=0.0, negative_label_downscaling=False, verbose=False, **kw)


def _inputs(B, Z, C, seed=0):
    z, eps, cl = R.planted(np.random.default_rng(seed + B * 1000 + Z), B, Z, C)
    return z[:, :Z], eps[:, :Z], cl


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("B,Z,C", SHAPES)
def test_reference_against_autograd_of_the_per_class_definition(B, Z, C):
    """L = sum_c (n_c / n) MMD^2(q_c, q_pooled) with MMD^2(p, q) = E_pp k - 2 E_pq k + E_qq k over the empirical distributions, written
    class by class in fp64 torch; its value and its gradient with respect to z against mmd_ref's sum_ij w_ij k_ij and g"""
    import torch
    z, _, cl = _inputs(B, Z, C)
    s2 = float(Z)
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    k = torch.exp(-((zt[:, None, :] - zt[None, :, :]) ** 2).sum(2) / (2 * s2))
    L = 0
    for c in np.unique(cl):
        m = torch.from_numpy(cl == c)
        n_c = int(m.sum())
        L = L + (n_c / B) * (k[m][:, m].mean() - 2 * k[m].mean() + k.mean())
    L.backward()
    L_rows, g, _, _ = R.mmd_ref(z, cl, s2)
    scale = max(1.0, float(zt.grad.abs().max()))
    assert abs(L_rows.sum() - float(L.detach())) <= 1e-14 and np.abs(g - zt.grad.numpy()).max() <= 1e-14 * scale
    assert L_rows.sum() >= -1e-15


@pytest.mark.parametrize("B,Z,C", SHAPES)
def test_linear_kernel_identity_with_the_between_class_variance(B, Z, C):
    """the same weights on z_i . z_j give sum_c (n_c / n) |m_c - m|^2: the numerator of class_leak's eta^2 summed over the dimensions"""
    z, _, cl = _inputs(B, Z, C)
    z = z.astype(np.float64)
    lin = (R.weights(cl) * (z @ z.T)).sum()
    m = z.mean(0)
    between = sum((cl == c).mean() * ((z[cl == c].mean(0) - m) ** 2).sum() for c in np.unique(cl))
    assert abs(lin - between) <= 1e-12 * max(1.0, between)


def test_a_single_class_gives_exact_zeros():
    z, _, _ = _inputs(9, 5, 1)
    for cid in (0, -4, 2147483647):
        cl = np.full(9, cid, np.int32)
        assert not R.weights(cl).any()
        L_rows, g, bL, bg = R.mmd_ref(z, cl, 5.0)
        assert not L_rows.any() and not g.any() and not bL.any() and not bg.any()


def test_invariance_under_a_permutation_of_the_rows():
    B, Z, C = 23, 7, 3
    z, _, cl = _inputs(B, Z, C)
    p = np.random.default_rng(5).permutation(B)
    L0, g0, _, _ = R.mmd_ref(z, cl, 3.5)
    L1, g1, _, _ = R.mmd_ref(z[p], cl[p], 3.5)
    assert np.abs(L1 - L0[p]).max() <= 1e-15 and np.abs(g1 - g0[p]).max() <= 1e-15
    assert abs(L1.sum() - L0.sum()) <= 1e-15


def test_planted_inputs_hold_what_they_promise():
    z, eps, cl = R.planted(np.random.default_rng(1), 67, 65, 5)
    assert z.shape == eps.shape == (67, 68) and np.isnan(z[:, 65:]).all() and np.isnan(eps[:, 65:]).all()
    assert np.isfinite(z[:, :65]).all() and np.isfinite(eps[:, :65]).all() and cl.dtype == np.int32
    ids, counts = np.unique(cl, return_counts=True)
    assert (ids < 0).any() and 1 in counts and (z[-1] == z[-2])[:65].all()
    assert z[cl == R.CLASS_IDS[0], :65].mean() - z[cl != R.CLASS_IDS[0], :65].mean() > 0.5


def test_apply_ref_is_the_latent_backward_of_the_summed_gradient():
    """the additions to d[mu | sigma] times Wl are what a larger dlat would have sent to d(enc_out): linearity, in fp64"""
    B, Z, De = 6, 5, 9
    rng = np.random.default_rng(2)
    z, eps, cl = _inputs(B, Z, 3)
    L_rows, g, _, bg = R.mmd_ref(z, cl, float(Z))
    Wl = rng.standard_normal((2 * Z, De)).astype(np.float32)
    dlat = rng.standard_normal((B, 2 * Z)).astype(np.float32)
    denc = (dlat.astype(np.float64) @ Wl.astype(np.float64))
    r = R.apply_ref(g, bg, eps, 12.5, Wl, dlat, denc, "bf16")
    assert np.abs(r["denc"] - r["dlat"] @ Wl.astype(np.float64)).max() <= 1e-12
    assert np.abs(r["add"][:, Z:] - r["add"][:, :Z] * eps).max() <= 1e-15 and (r["denc_bound"] > 0).all()


# ------------------------------------------------------------------------------------------ the score
def test_class_mmd_score():
    from musicstyletransfer_amd.step_math import class_mmd_score
    assert class_mmd_score([0.75, 3.0, 0.0]) == dict(class_mmd=0.25, class_mmd_bad=0)
    s = class_mmd_score(np.array([0.0, 0.0, 2.0]))
    assert math.isnan(s["class_mmd"]) and s["class_mmd_bad"] == 2 and isinstance(s["class_mmd_bad"], int)
    with pytest.raises(ValueError):
        class_mmd_score([1.0, 2.0])


def test_step_math_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None\n"
            "from musicstyletransfer_amd import step_math as S\n"
            "assert S.class_mmd_score([1.0, 2.0, 0.0])['class_mmd'] == 0.5\n"
            "S.check_class_mmd(10.0, 0.0)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------ flags and config
def test_flags_and_train_config():
    from musicstyletransfer_amd.VarAutoEncoder import config, main
    d = config.get_config([])
    assert d.class_mmd == 0.0 and d.class_mmd_bandwidth == 0.0
    args = config.get_config(["--class-mmd", "250", "--class-mmd-bandwidth", "16"])
    assert args.class_mmd == 250.0 and args.class_mmd_bandwidth == 16.0
    tc = main.create_train_config(args)
    assert tc.class_mmd == 250.0 and tc.class_mmd_bandwidth == 16.0 and main.create_train_config(d).class_mmd == 0.0
    assert main.create_toy_train_config(class_mmd=100.0).class_mmd == 100.0 and main.create_toy_train_config().class_mmd == 0.0


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf")])
def test_train_config_refuses_a_negative_or_non_finite_multiplier(bad):
    with pytest.raises(ValueError, match="class_mmd"):
        _train_config(class_mmd=bad)
    with pytest.raises(ValueError, match="class_mmd"):
        _train_config(class_mmd=1.0, class_mmd_bandwidth=bad)


def test_train_config_yaml_round_trip(tmp_path):
    from musicstyletransfer_amd.VarAutoEncoder import config
    tc = _train_config(class_mmd=300.0)
    f = str(tmp_path / "train.yaml")
    tc.save(f)
    back = config.Config.load(f)
    assert back == tc and back.class_mmd == 300.0
    lines = [ln for ln in open(f).read().splitlines() if not ln.startswith("class_mmd")]
    old = str(tmp_path / "old.yaml")
    open(old, "w").write("\n".join(lines) + "\n")
    back = config.Config.load(old)  # a file written before the fields existed: off
    assert back.class_mmd == 0.0 and back.class_mmd_bandwidth == 0.0 and back == _train_config()


def test_train_script_documents_the_flag():
    text = open(os.path.join(ROOT, "scripts", "train-vae.sh")).read()
    assert "--class-mmd LAMBDA" in text and '"$@"' in text


# ------------------------------------------------------------------------------------------ ABI
def test_header_declares_mst_class_mmd(lib):
    from musicstyletransfer_amd import _lib
    assert "mst_class_mmd(" in open(os.path.join(ROOT, "include", "mst_hip.h")).read()
    assert hasattr(lib, "mst_class_mmd") and lib.mst_version() >= 123
    assert len(_lib.STRUCTS) == 12  # plain arguments only: no new struct
    ci, ci64, vp, f32 = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES["mst_class_mmd"] == (ci, [ci, ci64, ci64, ci64, vp, ci64, vp, ci64, vp, f32, f32, vp, vp, vp, ci64, vp, vp, vp, vp])


#          dtype B  Z  De  z   ldz eps ldeps cl  s2   coef Wl  dlat denc stride rows tick acc
_VALUE = (0, 3, 4, 1, 64, 4, None, 0, 64, 4.0, 0.0, None, None, None, 0, 64, 64, 64)
_GRAD = (0, 3, 4, 8, 64, 4, 64, 4, 64, 4.0, 2.0, 64, 64, 64, 8, 64, 64, 64)


def _with(base, **kw):
    names = ("dtype", "B", "Z", "De", "z", "ld_z", "eps", "ld_eps", "classes", "s2", "coef", "Wl", "dlat", "d_enc_out", "stride", "rows",
             "ticket", "acc")
    a = dict(zip(names, base))
    a.update(kw)
    return tuple(a[n] for n in names)


@pytest.mark.parametrize("what,args", [
    ("null z", _with(_VALUE, z=None)), ("null classes", _with(_VALUE, classes=None)), ("null rows", _with(_VALUE, rows=None)),
    ("null ticket", _with(_VALUE, ticket=None)), ("null acc", _with(_VALUE, acc=None)),
    ("B = 0", _with(_VALUE, B=0)), ("negative B", _with(_VALUE, B=-3)), ("Z = 0", _with(_VALUE, Z=0)), ("De = 0", _with(_VALUE, De=0)),
    ("ld_z < Z", _with(_VALUE, ld_z=3)), ("s2 = 0", _with(_VALUE, s2=0.0)), ("negative s2", _with(_VALUE, s2=-1.0)),
    ("s2 NaN", _with(_VALUE, s2=float("nan"))), ("s2 inf", _with(_VALUE, s2=float("inf"))), ("coef NaN", _with(_VALUE, coef=float("nan"))),
    ("coef inf", _with(_GRAD, coef=float("inf"))),
    ("dlat without Wl", _with(_GRAD, Wl=None)), ("dlat without d_enc_out", _with(_GRAD, d_enc_out=None)),
    ("dlat without eps", _with(_GRAD, eps=None)), ("Wl without dlat", _with(_GRAD, dlat=None)),
    ("eps without dlat", _with(_VALUE, eps=64, ld_eps=4)),
    ("gradient with dtype fp32", _with(_GRAD, dtype=2)), ("gradient with dtype 7", _with(_GRAD, dtype=7)),
    ("ld_eps < Z", _with(_GRAD, ld_eps=3)), ("stride < De", _with(_GRAD, stride=7)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_bad_arguments_are_refused_before_any_hip_call(lib, what, args):
    """(the pointers are never followed and there is no device here: the checks come first)"""
    rc = lib.mst_class_mmd(*args, None)
    assert rc != 0 and b"mst_class_mmd" in lib.mst_last_error(), what
