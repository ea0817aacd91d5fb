"""Clipping by the global gradient norm on the host side: engine.clip_scale — the one host statement of the factor the device applies
(the clipping group of mst_adam_args) —, the refused values, the flag, TrainConfig's YAML round trip, and the argument checks of the two entry points,
which happen before any HIP call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _train_config(**kw):
    from musicstyletransfer_amd.VarAutoEncoder import trainer
    return trainer.TrainConfig(batch_size=8, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                               optimizer=trainer.OptimizerConfig(learning_rate=3e-4, optimizer="adam", optimizer_params="clip_gradient:1.0"),
                               kl_loss=0.5, label_smoothing=0.0, negative_label_downscaling=False, verbose=False, **kw)


def test_clip_scale_known_answers():
    from musicstyletransfer_amd import engine as E
    c = E.clip_scale(5.0, 5.0)  # 5 + 1e-8f is 5 in fp32: at the bound nothing is clipped
    assert c == 1 and isinstance(c, np.float32)
    c = E.clip_scale(10.0, 5.0)
    assert isinstance(c, np.float32) and c == np.float32(5) / np.float32(10) == np.float32(0.5)
    assert E.clip_scale(3.0, 1e6) == 1 and E.clip_scale(0.0, 1.0) == 1  # far below the bound; a zero gradient (1 / 1e-8 > 1)
    # np.float32 arithmetic, not double: the quotient is the fp32 one
    c = E.clip_scale(3.0, 1.0)
    assert c == np.float32(1) / np.float32(3) and float(c) != 1.0 / 3.0


def test_clip_refs_agree_with_clip_scale():
    import clip_refs as R
    from musicstyletransfer_amd import engine as E
    g = np.random.default_rng(3).standard_normal(1001) * 7
    S = R.sumsq(g, 400, 1 / 64, 1 / 65536)
    assert abs(S - (np.sum((g[:400] / 64) ** 2) + np.sum((g[400:] / 65536) ** 2))) <= 1e-12 * S
    norm, c = R.norm_and_scale(S, 0.5 * np.sqrt(S))
    assert abs(c - float(E.clip_scale(norm, 0.5 * norm))) <= 2.0 ** -22 and abs(c - 0.5) <= 1e-7
    assert R.norm_and_scale(S, 2 * np.sqrt(S))[1] == 1.0
    assert R.sumsq_bound(2 ** 21 + 3, 256) == (33 + 16) * 2.0 ** -24 and R.sumsq_bound(5, 256) == 17 * 2.0 ** -24


@pytest.mark.parametrize("bad", [-1.0, -1e-9, float("inf"), float("-inf"), float("nan")])
def test_check_clip_refuses(bad):
    from musicstyletransfer_amd import engine as E
    with pytest.raises(ValueError):
        E.check_clip(bad)
    with pytest.raises(ValueError):
        _train_config(clip_global_norm=bad)


def test_check_clip_accepts():
    from musicstyletransfer_amd import engine as E
    for ok in (0, 0.0, 1e-3, 1.0, 250):
        E.check_clip(ok)
    E.check_clip()


def test_flag_default_and_parsing():
    from musicstyletransfer_amd.VarAutoEncoder import config, main
    a = config.get_config([])
    assert a.clip_global_norm == 0.0 and main.create_train_config(a).clip_global_norm == 0.0
    a = config.get_config(["--clip-global-norm", "1.5"])
    assert a.clip_global_norm == 1.5 and isinstance(a.clip_global_norm, float)
    assert main.create_train_config(a).clip_global_norm == 1.5  # main.py passes it through
    assert main.create_toy_train_config(3, clip_global_norm=2.0).clip_global_norm == 2.0
    with pytest.raises(SystemExit):
        config.get_config(["--clip-global-norm", "tight"])


def test_train_config_yaml_round_trip(tmp_path):
    from musicstyletransfer_amd.VarAutoEncoder import config
    tc = _train_config(clip_global_norm=1.25)
    f = str(tmp_path / "train.yaml")
    tc.save(f)
    back = config.Config.load(f)
    assert back == tc and back.clip_global_norm == 1.25 and back.kl_loss_weight == 0.5
    # a file written before the field existed: it loads with 0 (off)
    text = open(f).read().splitlines()
    lines = [ln for ln in text if not ln.startswith("clip_global_norm:")]
    assert len(lines) == len(text) - 1
    old = str(tmp_path / "old.yaml")
    open(old, "w").write("\n".join(lines) + "\n")
    back = config.Config.load(old)
    assert back.clip_global_norm == 0.0 and back == _train_config()


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    G = lib.mst_grad_sumsq_parts()
    assert 0 < G <= 256 and G == lib.mst_grad_sumsq_parts()
    one = 16  # a non-NULL, 16-byte aligned stand-in: every call below is refused before anything is read
    assert lib.mst_grad_sumsq(0, one, 0, 1.0, 1.0, one, None) == -1
    assert lib.mst_grad_sumsq(8, None, 0, 1.0, 1.0, one, None) == -1 and lib.mst_grad_sumsq(8, one, 0, 1.0, 1.0, None, None) == -1
    assert lib.mst_grad_sumsq(8, one, 9, 1.0, 1.0, one, None) == -1 and lib.mst_grad_sumsq(8, one, -1, 1.0, 1.0, one, None) == -1
    assert b"mst_grad_sumsq" in lib.mst_last_error()
    assert lib.mst_grad_sumsq(8, 20, 4, 1.0, 1.0, one, None) == -1 and b"aligned" in lib.mst_last_error()

    def gnorm(parts=one, n_parts=G, max_norm=1.0, **kw):
        q = _lib.AdamArgs(dtype=_lib.MST_BF16, n=8, w=one, grad=one, m=one, v=one, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, rescale=1.0, clip=-1.0,
                          parts=parts, n_parts=n_parts, max_norm=max_norm, **kw)
        return lib.mst_adam_flat(q, None)

    assert gnorm(parts=None) == -1 and b"parts" in lib.mst_last_error()
    # the other fields of the group without parts are refused too, not ignored
    assert gnorm(parts=None, n_parts=0) == -1 and b"parts" in lib.mst_last_error()  # (max_norm alone)
    assert gnorm(parts=None, max_norm=0.0) == -1 and b"parts" in lib.mst_last_error()  # (n_parts alone)
    assert gnorm(parts=None, n_parts=0, max_norm=0.0, gstat=one) == -1 and b"parts" in lib.mst_last_error()
    assert gnorm(n_parts=G - 1) == -1 and gnorm(n_parts=0) == -1 and b"mst_grad_sumsq_parts" in lib.mst_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert gnorm(max_norm=bad) == -1 and b"max_norm" in lib.mst_last_error(), bad
    assert gnorm(parts=20) == -1 and b"aligned" in lib.mst_last_error()
    # the step count of a clipped launch is mst_step_begin's
    assert gnorm(step_state=one, advance_step=1) == -1 and b"advance_step" in lib.mst_last_error()
    assert gnorm() == -1 and b"mst_adam_flat: bad argument" in lib.mst_last_error()  # (null step_state: the launch's own checks follow)
    assert lib.mst_adam_flat(None, None) == -1 and b"mst_adam_flat" in lib.mst_last_error()
    with pytest.raises(_lib.MstError):
        _lib.call("mst_grad_sumsq", 0, None, 0, 1.0, 1.0, None, None)
