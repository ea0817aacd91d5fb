"""The exponential moving average of the weights on the host side: engine.ema_decay_at and engine.ema_update — the one host
statement of what the Adam launch computes in its averaging form (mst_adam_args.ema) —, the refused values, the flag, TrainConfig's YAML
round trip, the plan's hyper-parameters with the option off, and the argument checks of the two entry points, which happen before any
HIP call."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32


def _train_config(**kw):
    from musicstyletransfer_amd.VarAutoEncoder import trainer
    return trainer.TrainConfig(batch_size=8, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                               optimizer=trainer.OptimizerConfig(learning_rate=3e-4, optimizer="adam", optimizer_params="clip_gradient:1.0"),
                               kl_loss=0.5, label_smoothing=0.0, negative_label_downscaling=False, verbose=False, **kw)


def test_ema_decay_at_hand_values():
    from musicstyletransfer_amd import engine as E
    d = E.ema_decay_at(1, 0.99)
    assert isinstance(d, np.float32) and d == F(2) / F(11) and d.tobytes() == (F(2) / F(11)).tobytes()
    assert E.ema_decay_at(2, 0.99) == F(3) / F(12) == F(0.25)
    # np.float32 arithmetic, not double
    assert float(E.ema_decay_at(1, 0.99)) != 2.0 / 11.0
    # the warm-up (1 + t) / (10 + t) reaches 0.99 at t = 890 (891 / 900 = 0.99): below it the warm-up, from there on the decay itself
    assert E.ema_decay_at(889, 0.99) == F(890) / F(899) < F(0.99)
    assert E.ema_decay_at(890, 0.99) == F(0.99) and E.ema_decay_at(891, 0.99) == F(0.99) and E.ema_decay_at(10 ** 6, 0.99) == F(0.99)
    # ... and 0.5 at t = 8 (9 / 18): t = 7 is 8 / 17 below it, t = 9 is capped
    assert E.ema_decay_at(7, 0.5) == F(8) / F(17) and E.ema_decay_at(8, 0.5) == F(0.5) and E.ema_decay_at(9, 0.5) == F(0.5)
    # the configured decay is taken as its fp32 value
    assert E.ema_decay_at(10 ** 6, 0.999) == F(0.999) and float(E.ema_decay_at(10 ** 6, 0.999)) != 0.999
    # monotone in t up to the cap
    ds = [E.ema_decay_at(t, 0.9) for t in range(1, 200)]
    assert all(a <= b for a, b in zip(ds, ds[1:])) and ds[-1] == F(0.9) and ds[0] < ds[40]


def test_ema_update_is_two_rounded_products_and_a_rounded_sum():
    from musicstyletransfer_amd import engine as E
    rng = np.random.default_rng(5)
    e, w = rng.standard_normal(4096).astype(F), rng.standard_normal(4096).astype(F)
    for d in (E.ema_decay_at(1, 0.99), E.ema_decay_at(300, 0.99), F(0.99), F(0.999)):
        got = E.ema_update(e, w, d)
        assert got.dtype == np.float32
        omd = F(1) - d
        want = np.array([F(F(d * a) + F(omd * b)) for a, b in zip(e, w)], F)  # element by element, every operation rounded to fp32
        assert got.tobytes() == want.tobytes()
        # the double-precision value of the same expression is within one rounding of the sum and half an ulp of each product
        exact = float(d) * e.astype(np.float64) + float(omd) * w.astype(np.float64)
        assert np.abs(got - exact).max() <= 2.0 ** -22 * np.abs(exact).max() + 2.0 ** -23 * (np.abs(e).max() + np.abs(w).max())
    # a fused multiply-add would differ somewhere on this many values: the statement is the unfused one
    d = F(0.99)
    fused = (float(d) * e.astype(np.float64) + (F(1) - d) * w).astype(F)  # (omd * w rounded, d * e exact, one rounding of the sum)
    assert (fused != E.ema_update(e, w, d)).any()
    assert E.ema_update(F(2.0), F(4.0), F(0.5)) == F(3.0)


def test_ema_update_fixed_points():
    """e == w stays where the two products are exact (then d e + (1 - d) e is e itself, and 1 - d is exact for d in [0.5, 1)): powers of
    two and zero under any such d, short mantissas under a dyadic d. For arbitrary values the products round, and e moves by at most one
    ulp: each product is within half an ulp of its own, smaller, magnitude, the sum rounds once."""
    from musicstyletransfer_amd import engine as E
    pow2 = np.array([0.0, -0.0, 1.0, -2.0, 2.0 ** -20, 2.0 ** 30, -(2.0 ** -100)], F)
    for d in (F(0.99), F(0.999), E.ema_decay_at(40, 0.99), F(0.5)):
        assert d >= 0.5 and E.ema_update(pow2, pow2, d).tobytes() == pow2.tobytes()
    short = np.array([3.0, -5.0, 0.375, 7.0, 1.25, -96.0], F)
    for d in (F(0.5), F(0.75), F(0.875)):
        assert E.ema_update(short, short, d).tobytes() == short.tobytes()
    x = np.random.default_rng(9).standard_normal(10000).astype(F)
    for d in (F(0.99), E.ema_decay_at(1, 0.99)):
        assert (np.abs(E.ema_update(x, x, d) - x) <= np.spacing(np.abs(x))).all()
    # and the average of a constant sequence of weights, started at that constant, never leaves it (the padding words of the bucket)
    e = pow2.copy()
    for t in range(1, 30):
        e = E.ema_update(e, pow2, E.ema_decay_at(t, 0.99))
    assert e.tobytes() == pow2.tobytes()


@pytest.mark.parametrize("bad", [-0.1, -1e-9, 1.0, 1.5, float("inf"), float("-inf"), float("nan")])
def test_check_ema_refuses(bad):
    from musicstyletransfer_amd import engine as E
    with pytest.raises(ValueError):
        E.check_ema(bad)
    with pytest.raises(ValueError):
        _train_config(ema_decay=bad)


def test_check_ema_accepts():
    from musicstyletransfer_amd import engine as E
    for ok in (0, 0.0, 1e-3, 0.5, 0.99, 0.9999):
        E.check_ema(ok)
    E.check_ema()


def test_flag_default_and_parsing():
    from musicstyletransfer_amd.VarAutoEncoder import config, main
    from musicstyletransfer_amd import generate
    a = config.get_config([])
    assert a.ema_decay == 0.0 and main.create_train_config(a).ema_decay == 0.0
    a = config.get_config(["--ema-decay", "0.995"])
    assert a.ema_decay == 0.995 and isinstance(a.ema_decay, float)
    assert main.create_train_config(a).ema_decay == 0.995  # main.py passes it through
    assert main.create_toy_train_config(3, ema_decay=0.9).ema_decay == 0.9
    with pytest.raises(SystemExit):
        config.get_config(["--ema-decay", "slow"])
    with pytest.raises(ValueError):
        main.create_train_config(config.get_config(["--ema-decay", "1.0"]))
    g = generate.build_parser().parse_args(["--model-output", "m", "--mode", "prior", "--out", "o"])
    assert g.ema is False
    assert generate.build_parser().parse_args(["--model-output", "m", "--mode", "prior", "--out", "o", "--ema"]).ema is True


def test_train_config_yaml_round_trip(tmp_path):
    from musicstyletransfer_amd.VarAutoEncoder import config
    tc = _train_config(ema_decay=0.995, clip_global_norm=1.25)
    f = str(tmp_path / "train.yaml")
    tc.save(f)
    back = config.Config.load(f)
    assert back == tc and back.ema_decay == 0.995 and back.clip_global_norm == 1.25
    # a file written before the field existed: it loads with 0 (off)
    text = open(f).read().splitlines()
    lines = [ln for ln in text if not ln.startswith("ema_decay:")]
    assert len(lines) == len(text) - 1
    old = str(tmp_path / "old.yaml")
    open(old, "w").write("\n".join(lines) + "\n")
    back = config.Config.load(old)
    assert back.ema_decay == 0.0 and back == _train_config(clip_global_norm=1.25)


def test_off_leaves_the_plans_hyper_parameters_as_they_were():
    """Trainer._initialize_optimizers needs no device: the keyword joins the plan's hyper-parameters — the plan cache's key — only when the
    option is on"""
    from musicstyletransfer_amd.VarAutoEncoder import trainer

    def hyper(**kw):
        t = trainer.Trainer.__new__(trainer.Trainer)
        t.config = _train_config(**kw)
        t._initialize_optimizers()
        return t

    off, zero, on = hyper(), hyper(ema_decay=0.0), hyper(ema_decay=0.99)
    want = dict(lr=3e-4, clip_gradient=1.0, kl_weight=0.5, label_smoothing=0.0, negative_label_downscaling=False, internal_eps=True)
    assert off.hyper == want and zero.hyper == want and list(off.hyper) == list(want)
    assert on.hyper == dict(want, ema_decay=0.99) and on.ema_decay == 0.99 and off.ema_decay == 0.0
    both = hyper(ema_decay=0.9, clip_global_norm=2.0, kl_warmup_steps=5)
    assert both.hyper["ema_decay"] == 0.9 and both.hyper["clip_global_norm"] == 2.0 and both.hyper["kl_warmup_steps"] == 5
    # a TrainConfig unpickled or loaded from before the field: off
    old = hyper()
    del old.config.__dict__["ema_decay"]
    old._initialize_optimizers()
    assert old.hyper == want and old.ema_decay == 0.0


def test_entry_points_reject_bad_arguments_before_any_hip_call():
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    assert lib.mst_version() >= 119  # 119: mst_adam_args; 112: mst_ema_swap
    G = lib.mst_grad_sumsq_parts()
    one = 16  # a non-NULL, 16-byte aligned stand-in: every call below is refused before anything is read

    def adam(ema=one, decay=0.99, parts=None, n_parts=0, max_norm=0.0, **kw):
        q = _lib.AdamArgs(dtype=_lib.MST_BF16, n=8, w=one, grad=one, m=one, v=one, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, rescale=1.0, clip=-1.0,
                          parts=parts, n_parts=n_parts, max_norm=max_norm, ema=ema, decay=decay, **kw)
        return lib.mst_adam_flat(q, None)

    assert adam(ema=None) == -1 and b"ema" in lib.mst_last_error()
    assert adam(ema=20) == -1 and b"aligned" in lib.mst_last_error()
    for bad in (0.0, -0.5, 1.0, 2.0, float("inf"), float("nan")):
        assert adam(decay=bad) == -1 and b"decay" in lib.mst_last_error(), bad
    assert adam(ema=None, decay=float("nan")) == -1 and b"ema" in lib.mst_last_error()
    # with parts, the checks of the clipping group
    assert adam(parts=one, n_parts=G - 1, max_norm=1.0) == -1 and b"mst_grad_sumsq_parts" in lib.mst_last_error()
    assert adam(parts=one, n_parts=G, max_norm=0.0) == -1 and b"max_norm" in lib.mst_last_error()
    assert adam(parts=20, n_parts=G, max_norm=1.0) == -1 and b"aligned" in lib.mst_last_error()
    # the step count of an averaging launch is mst_step_begin's
    assert adam(step_state=one, advance_step=1) == -1 and b"advance_step" in lib.mst_last_error()
    assert adam() == -1 and b"mst_adam_flat: bad argument" in lib.mst_last_error()  # (null step_state: the launch's own checks follow)
    assert adam(parts=one, n_parts=G, max_norm=1.0) == -1 and b"mst_adam_flat: bad argument" in lib.mst_last_error()

    swap = lambda n=8, w=one, ema=32, w16=64: lib.mst_ema_swap(_lib.MST_BF16, n, w, ema, w16, None)
    assert swap(n=0) == -1 and swap(w=None) == -1 and swap(ema=None) == -1 and b"mst_ema_swap" in lib.mst_last_error()
    assert swap(ema=one) == -1 and b"distinct" in lib.mst_last_error()
    assert swap(w=20) == -1 and swap(ema=40) == -1 and swap(w16=66) == -1 and b"aligned" in lib.mst_last_error()
    assert lib.mst_ema_swap(7, 8, one, 32, 64, None) != 0  # an unknown activation type
