"""Training schedules on the host side: the flags, TrainConfig's YAML round trip, the refused combinations and known answers of
engine.schedule_values — the one host statement of the formulas the device evaluates from Adam's step count (step_begin.hpp)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("kl_warmup_steps", "kl_cycle_steps", "kl_free_bits", "lr_warmup_steps")


def _train_config(**kw):
    from musicstyletransfer_amd.VarAutoEncoder import trainer
    return trainer.TrainConfig(batch_size=8, sampling_frequency=0, checkpoint_frequency=0, num_checkpoints_not_improved=-1,
                               optimizer=trainer.OptimizerConfig(learning_rate=3e-4, optimizer="adam", optimizer_params="clip_gradient:1.0"),
                               kl_loss=0.5, label_smoothing=0.0, negative_label_downscaling=False, verbose=False, **kw)


def test_flag_defaults_and_parsing():
    from musicstyletransfer_amd.VarAutoEncoder import config, main
    a = config.get_config([])
    assert [getattr(a, n) for n in NAMES] == [0, 0, 0.0, 0]
    a = config.get_config(["--kl-warmup-steps", "2000", "--kl-cycle-steps", "5000", "--kl-free-bits", "8", "--lr-warmup-steps", "500"])
    assert [getattr(a, n) for n in NAMES] == [2000, 5000, 8.0, 500]
    assert isinstance(a.kl_free_bits, float) and isinstance(a.kl_warmup_steps, int)
    tc = main.create_train_config(a)  # main.py passes them through
    assert [getattr(tc, n) for n in NAMES] == [2000, 5000, 8.0, 500]
    with pytest.raises(SystemExit):
        config.get_config(["--kl-warmup-steps", "1.5"])


def test_train_config_yaml_round_trip(tmp_path):
    from musicstyletransfer_amd.VarAutoEncoder import config
    tc = _train_config(kl_warmup_steps=4, kl_cycle_steps=6, kl_free_bits=2.5, lr_warmup_steps=5)
    f = str(tmp_path / "train.yaml")
    tc.save(f)
    back = config.Config.load(f)
    assert back == tc and [getattr(back, n) for n in NAMES] == [4, 6, 2.5, 5]
    assert back.optimizer.learning_rate == 3e-4 and back.kl_loss_weight == 0.5
    # a file written before the fields existed: they load with their defaults
    lines = [ln for ln in open(f).read().splitlines() if not any(ln.startswith(n + ":") for n in NAMES)]
    assert len(lines) == len(open(f).read().splitlines()) - 4
    old = str(tmp_path / "old.yaml")
    open(old, "w").write("\n".join(lines) + "\n")
    back = config.Config.load(old)
    assert [getattr(back, n) for n in NAMES] == [0, 0, 0.0, 0]
    assert back == _train_config()


@pytest.mark.parametrize("kw", [dict(kl_warmup_steps=-1), dict(kl_cycle_steps=-2, kl_warmup_steps=1), dict(kl_free_bits=-0.5),
                                dict(lr_warmup_steps=-3), dict(kl_cycle_steps=6), dict(kl_cycle_steps=6, kl_warmup_steps=7),
                                dict(kl_free_bits=float("nan"))])
def test_invalid_combinations_raise(kw):
    from musicstyletransfer_amd import engine as E
    with pytest.raises(ValueError):
        E.check_schedule(**kw)
    with pytest.raises(ValueError):
        _train_config(**kw)


def test_valid_combinations_pass():
    from musicstyletransfer_amd import engine as E
    for kw in (dict(), dict(kl_warmup_steps=6, kl_cycle_steps=6), dict(kl_warmup_steps=4, kl_cycle_steps=6, kl_free_bits=8.0, lr_warmup_steps=5),
               dict(kl_free_bits=0.25), dict(lr_warmup_steps=1)):
        E.check_schedule(**kw)


def test_schedule_values_known_answers():
    """W_b = 4, C = 6, W_lr = 5 over t = 1..15: the ramp, the plateau, the restarts at t = 7 and 13, and f_lr reaching 1 at t = 5"""
    from musicstyletransfer_amd import engine as E
    ramp = [0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 0.25, 0.5, 0.75, 1.0, 1.0, 1.0, 0.25, 0.5, 0.75]
    f_lr = [0.2, 0.4, 0.6, 0.8, 1.0] + [1.0] * 10
    for t in range(1, 16):
        beta, f = E.schedule_values(t, kl_weight=0.5, kl_warmup_steps=4, kl_cycle_steps=6, lr_warmup_steps=5)
        assert beta == 0.5 * ramp[t - 1] and f == f_lr[t - 1], t  # (binary fractions of 0.5; t / 5 is the correctly rounded quotient)
    # beta_t is an fp32 value: fp32(fp32(kl_weight) * ramp), one rounding of the double product
    beta, _ = E.schedule_values(1, kl_weight=0.3, kl_warmup_steps=3)
    assert beta == float(np.float32(float(np.float32(0.3)) * (1 / 3))) and beta == float(np.float32(beta))
    # no cycle: the ramp never restarts; everything off: the constants
    assert [E.schedule_values(t, 2.0, kl_warmup_steps=4)[0] for t in (1, 4, 5, 400)] == [0.5, 2.0, 2.0, 2.0]
    assert E.schedule_values(7, 0.7) == (float(np.float32(0.7)), 1.0)
    assert E.schedule_values(3, 1.0, lr_warmup_steps=2) == (1.0, 1.0)
