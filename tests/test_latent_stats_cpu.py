"""Per-dimension latent statistics without a GPU: the two host formulations of the accumulator (tests/latent_stats_refs.py) against
each other and on known answers, engine.latent_scores on sums worked by hand, the ABI (mst_latent_dim_stats, version 120, no new
struct, every refusal before any HIP call), the --latent-stats flag and TrainConfig's YAML round trip."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_stats_refs as R  # noqa: E402


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


# ------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("B,Z,C", [(1, 1, 1), (5, 3, 2), (67, 65, 5)])
def test_the_loop_and_the_whole_array_sums_agree(B, Z, C):
    """finite inputs (the two may differ in the last bits of a sum): counts equal, every other cell within the distance of two
    summation orders of the same B terms, 2 (B - 1) 2^-53 sum |term|"""
    rng = np.random.default_rng(B * 1000 + Z)
    mu = rng.standard_normal((B, Z)).astype(np.float32)
    sg = (np.exp(rng.uniform(-1.5, 1.0, (B, Z))) * np.where(rng.random((B, Z)) < 0.25, -1, 1)).astype(np.float32)
    cl = rng.integers(0, C, B).astype(np.int32)
    a, b = R.dim_stats_ref(mu, sg, cl, C), R.dim_stats_vec(mu, sg, cl, C)
    assert np.array_equal(a[:, 0], b[:, 0]) and a[:, 0].sum() == B * Z
    tol = 2 * max(B - 1, 0) * 2.0 ** -53 * R.abs_sums(mu, sg, cl, C)
    assert (np.abs(a - b) <= tol).all(), float(np.abs(a - b).max())
    if B > 1:
        assert a[:, 4].sum() > 0 and np.abs(a[:, 1]).sum() > 0


def test_the_reference_on_a_batch_worked_by_hand():
    """five samples, two dimensions, every skip rule once; planes 0-3 are small dyadic numbers, exact in any order (plane 4 to an ulp
    of the logarithm: 1e-15)"""
    mu = np.array([[0.5, 2.0], [1.5, np.nan], [-1.0, 4.0], [8.0, 8.0], [0.25, 0.25]], np.float32)
    sg = np.array([[1.0, -2.0], [2.0, 1.0], [0.0, np.inf], [1.0, 1.0], [1.0, -0.0]], np.float32)
    cl = np.array([0, 1, 1, 2, -1], np.int32)  # (C = 2: the fourth sample's class is C, the fifth's -1)
    for f in (R.dim_stats_ref, R.dim_stats_vec):
        acc = f(mu, sg, cl, 2)
        assert acc.shape == (2, 5, 2) and acc.dtype == np.float64
        # class 0: sample 0 in both dimensions
        assert acc[0, :4].tolist() == [[1, 1], [0.5, 2.0], [0.25, 4.0], [1.0, 4.0]]
        assert acc[0, 4, 0] == 0.5 * (1.0 + 0.25 - 1.0 - 0.0) and abs(acc[0, 4, 1] - 0.5 * (4.0 + 4.0 - 1.0 - math.log(4.0))) <= 1e-15
        # class 1: sample 1 in dimension 0 only (NaN mu in dimension 1); sample 2 in neither (sigma 0, sigma inf)
        assert acc[1, :4].tolist() == [[1, 0], [1.5, 0], [2.25, 0], [4.0, 0]]
        assert abs(acc[1, 4, 0] - 0.5 * (4.0 + 2.25 - 1.0 - math.log(4.0))) <= 1e-15 and acc[1, 4, 1] == 0


def test_planted_inputs_hold_what_the_gpu_test_relies_on():
    mu, sg, cl = R.planted(np.random.default_rng(5), 67, 65, 5)
    Z = 65
    assert mu.shape == (67, 68) and np.isnan(mu[:, Z:]).all() and np.isnan(sg[:, Z:]).all()
    assert (sg[:, :Z] < 0).any() and (sg[:, :Z] == 0).sum() == 2 and np.isnan(mu[:, :Z]).sum() == 1 and np.isinf(sg[:, :Z]).sum() == 1
    assert (cl == -1).sum() == 1 and (cl == 5).sum() == 1
    acc = R.dim_stats_ref(mu[:, :Z], sg[:, :Z], cl, 5)
    # 65 samples of a class in range, at most four of their terms planted away; every sum finite although the inputs are not
    assert np.isfinite(acc).all() and 65 * 65 - 4 <= acc[:, 0].sum() == R._counted(mu[:, :Z], sg[:, :Z], cl, 5).sum() <= 65 * 65


# ------------------------------------------------------------------------------------------ latent_scores
def _hand_sums():
    """two classes of four samples, Z = 4. dim 0: mu = +-0.5 in each class alike (V = 0.25, nothing between the classes); dim 1:
    mu = +1 for class 0, -1 for class 1 (V = 1, all of it between the classes); dim 2: mu = +-0.01 (V = 1e-4, a hundredth of the
    threshold); dim 3: no sample counted. sigma = 0.5 everywhere; kl_d from the formula."""
    mus = {0: np.array([[0.5, 1.0, 0.01], [-0.5, 1.0, -0.01], [0.5, 1.0, 0.01], [-0.5, 1.0, -0.01]]),
           1: np.array([[0.5, -1.0, 0.01], [-0.5, -1.0, -0.01], [-0.5, -1.0, 0.01], [0.5, -1.0, -0.01]])}
    acc = np.zeros((2, 5, 4))
    for c, m in mus.items():
        kl = 0.5 * (0.25 + m * m - 1.0 - math.log(0.25))
        acc[c, 0, :3], acc[c, 1, :3], acc[c, 2, :3], acc[c, 3, :3], acc[c, 4, :3] = 4, m.sum(0), (m * m).sum(0), 4 * 0.25, kl.sum(0)
    return acc


def test_latent_scores_on_sums_worked_by_hand():
    from musicstyletransfer_amd.engine import latent_scores
    acc = _hand_sums()
    s = latent_scores(acc)
    assert s["active_units"] == 2 and isinstance(s["active_units"], int)
    assert abs(s["class_leak"] - 1.0) <= 1e-12
    base = 0.5 * (0.25 - 1.0 - math.log(0.25))
    want = [base + 0.5 * 0.25, base + 0.5 * 1.0, base + 0.5 * 1e-4]
    assert np.allclose(s["kl_dims"][:3], want, rtol=0, atol=1e-12) and math.isnan(s["kl_dims"][3]) and s["kl_dims"].shape == (4,)
    assert abs(s["kl_dim_max"] - want[1]) <= 1e-12 and s["kl_dims_used"] == 3
    assert abs(s["sigma_rms"] - 0.5) <= 1e-12
    # dim 0 alone (dimension 1 removed): active, and nothing of its variance lies between the classes
    only0 = acc.copy()
    only0[:, :, 1] = 0
    s0 = latent_scores(only0)
    assert s0["active_units"] == 1 and abs(s0["class_leak"]) <= 1e-12
    # the threshold is a parameter: at 1e-5 dimension 2 (V = 1e-4) is active too, and as free of the class as dimension 0
    s2 = latent_scores(only0, threshold=1e-5)
    assert s2["active_units"] == 2 and abs(s2["class_leak"]) <= 1e-12
    # nothing counted at all
    z = latent_scores(np.zeros((2, 5, 4)))
    assert z["active_units"] == 0 and z["kl_dims_used"] == 0 and np.isnan(z["kl_dims"]).all()
    assert all(math.isnan(z[k]) for k in ("class_leak", "kl_dim_max", "sigma_rms"))


def test_a_single_class_has_no_class_leak():
    from musicstyletransfer_amd.engine import latent_scores
    acc = _hand_sums()
    one = acc[:1]                       # one class in the table
    s = latent_scores(one)
    assert s["active_units"] == 1 and math.isnan(s["class_leak"])  # (within class 0, dimension 1 is constant)
    emptied = acc.copy()
    emptied[1] = 0                      # two classes in the table, samples of one only
    s = latent_scores(emptied)
    assert s["active_units"] == 1 and math.isnan(s["class_leak"])
    with pytest.raises(ValueError):
        latent_scores(np.zeros((2, 4, 4)))


def test_latent_scores_of_the_reference_sums():
    """a class that shifts dimension 0 by 3 sigma of the within-class spread: eta^2 = between / total, computed here from the samples"""
    from musicstyletransfer_amd.engine import latent_scores
    rng = np.random.default_rng(2)
    B, Z = 64, 3
    cl = (np.arange(B) % 2).astype(np.int32)
    mu = rng.standard_normal((B, Z)).astype(np.float32)
    mu[:, 0] += 3.0 * cl
    mu[:, 2] *= 0.01
    sg = np.full((B, Z), 0.5, np.float32)
    s = latent_scores(R.dim_stats_ref(mu, sg, cl, 2))
    m64 = mu.astype(np.float64)
    var = m64.var(0)
    eta = [sum((cl == c).mean() * (m64[cl == c, d].mean() - m64[:, d].mean()) ** 2 for c in (0, 1)) / var[d] for d in range(Z)]
    assert s["active_units"] == 2 and abs(s["class_leak"] - max(eta[0], eta[1])) <= 1e-12 and 0.5 < s["class_leak"] < 1


# ------------------------------------------------------------------------------------------ ABI
def test_abi_120(lib):
    from musicstyletransfer_amd import _lib
    assert hasattr(lib, "mst_latent_dim_stats") and lib.mst_version() >= 120
    assert len(_lib.STRUCTS) == 12  # plain arguments only: no new struct
    ci64, vp = ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["mst_latent_dim_stats"] == (ctypes.c_int, [ci64, ci64, ci64, vp, ci64, vp, ci64, vp, vp, vp])


@pytest.mark.parametrize("what,args", [
    ("B = 0", (0, 4, 2, 64, 4, 64, 4, 64, 64)),
    ("Z = 0", (3, 0, 2, 64, 4, 64, 4, 64, 64)),
    ("C = 0", (3, 4, 0, 64, 4, 64, 4, 64, 64)),
    ("negative B", (-3, 4, 2, 64, 4, 64, 4, 64, 64)),
    ("ld_mu < Z", (3, 4, 2, 64, 3, 64, 4, 64, 64)),
    ("ld_sigma < Z", (3, 4, 2, 64, 4, 64, 3, 64, 64)),
    ("null mu", (3, 4, 2, None, 4, 64, 4, 64, 64)),
    ("null sigma", (3, 4, 2, 64, 4, None, 4, 64, 64)),
    ("null classes", (3, 4, 2, 64, 4, 64, 4, None, 64)),
    ("null acc", (3, 4, 2, 64, 4, 64, 4, 64, None)),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_bad_arguments_are_refused_before_any_launch(lib, what, args):
    """(the pointers are never followed: the checks come first)"""
    rc = lib.mst_latent_dim_stats(*args, None)
    assert rc != 0 and b"mst_latent_dim_stats" in lib.mst_last_error(), what


# ------------------------------------------------------------------------------------------ flag and config
def test_flag_and_train_config():
    from musicstyletransfer_amd.VarAutoEncoder import config, main
    assert config.get_config([]).latent_stats is False
    args = config.get_config(["--latent-stats"])
    assert args.latent_stats is True
    assert main.create_train_config(args).latent_stats is True and main.create_train_config(config.get_config([])).latent_stats is False
    assert main.create_toy_train_config(latent_stats=True).latent_stats is True and main.create_toy_train_config().latent_stats is False


def test_train_config_yaml_round_trip(tmp_path):
    from musicstyletransfer_amd.VarAutoEncoder import config
    tc = _train_config(latent_stats=True)
    f = str(tmp_path / "train.yaml")
    tc.save(f)
    back = config.Config.load(f)
    assert back == tc and back.latent_stats is True and back.kl_loss_weight == 0.5
    # a file written before the field existed: it loads with False (off)
    text = open(f).read().splitlines()
    lines = [ln for ln in text if not ln.startswith("latent_stats:")]
    assert len(lines) == len(text) - 1
    old = str(tmp_path / "old.yaml")
    open(old, "w").write("\n".join(lines) + "\n")
    back = config.Config.load(old)
    assert back.latent_stats is False and back == _train_config()
