"""Decoder-input dropout without a GPU: the ABI (the trailing fields of mst_step_begin_args, the keep parameter of the two embedding entry
points, version 118), every refusal of mst_step_begin's job before any HIP call, engine.check_input_dropout, the flag, TrainConfig's
YAML round trip, and the references of tests/input_drop_refs.py on known answers."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_drop_refs as R  # noqa: E402


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


# ---------------------------------------------------------------------------------------------- the ABI
def test_the_abi_carries_the_job(lib):
    from musicstyletransfer_amd import _lib
    vp = ctypes.c_void_p
    assert lib.mst_version() >= 118
    assert len(_lib.STRUCTS) == 12  # fields of an existing struct, no new one (the twelfth is ABI 119's mst_adam_args)
    fields = _lib.StepBeginArgs._fields_
    assert [n for n, _ in fields[-10:]] == ["in_keep", "in_n", "in_p", "in_site", "in_index0", "in_src", "in_ld_src", "in_dst", "in_ld_dst",
                                            "in_row_bytes"]
    assert [t for _, t in fields[-10:]] == [vp, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32, ctypes.c_int64, vp, ctypes.c_int64, vp,
                                            ctypes.c_int64, ctypes.c_int64]
    assert fields[-11][0] == "sched_lr_warmup"  # appended behind the schedules
    for name, n_args in (("mst_embed_fwd", 20), ("mst_embed_bwd", 17)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n_args and args[-2:] == [vp, vp], (name, args)  # ..., keep, stream
    assert _lib.SIGNATURES["mst_embed_fwd"][1][-3] == vp  # (keymask, in front of keep)
    assert _lib.SIGNATURES["mst_embed_bwd"][1][-3] is ctypes.c_int64  # (s_off)
    from musicstyletransfer_amd import ops
    assert ops.IN_SITE == R.IN_SITE == 0x7FFF0001


# ---------------------------------------------------------------------------------------------- refusals
def _begin(lib, **over):
    """an mst_step_begin call whose job is valid (pointers are never followed: every use below is refused before any HIP call)"""
    from musicstyletransfer_amd import _lib
    q = _lib.StepBeginArgs()
    a = dict(rng_state=4096, in_keep=4096, in_n=76, in_p=0.25, in_site=R.IN_SITE, in_index0=38, in_src=8192, in_ld_src=48, in_dst=16384,
             in_ld_dst=48, in_row_bytes=40, sched=4096)  # (a schedule block without adam_state: the refusal a VALID job ends in)
    a.update(over)
    for k, v in a.items():
        setattr(q, k, v)
    return lib.mst_step_begin(ctypes.byref(q), None)


def test_a_valid_job_passes_its_checks(lib):
    # (the stand-in call is refused by a check that comes AFTER the job's, so nothing is launched here either)
    assert _begin(lib) == -1 and b"Adam's step count" in lib.mst_last_error()
    assert _begin(lib, in_src=None, in_dst=None) == -1 and b"Adam's step count" in lib.mst_last_error()  # the draw alone
    assert _begin(lib, in_p=0.0) == -1 and b"Adam's step count" in lib.mst_last_error()
    assert _begin(lib, in_p=1.0) == -1 and b"Adam's step count" in lib.mst_last_error()  # p = 1 is allowed
    assert _begin(lib, in_index0=0, in_n=2 ** 31 - 1) == -1 and b"Adam's step count" in lib.mst_last_error()
    # without in_keep the other fields are not looked at
    assert _begin(lib, in_keep=None, in_p=7.0, in_n=-1, in_ld_src=3) == -1 and b"Adam's step count" in lib.mst_last_error()


@pytest.mark.parametrize("over,text", [
    (dict(rng_state=None), b"needs the rng state"),
    (dict(in_p=-0.01), b"in_p"), (dict(in_p=1.01), b"in_p"), (dict(in_p=float("nan")), b"in_p"), (dict(in_p=float("inf")), b"in_p"),
    (dict(in_n=0), b"in_n"), (dict(in_n=-5), b"in_n"), (dict(in_n=2 ** 31), b"in_n"),
    (dict(in_index0=-1), b"in_index0"), (dict(in_index0=2 ** 31 - 76), b"below 2^31"), (dict(in_index0=2 ** 40), b"below 2^31"),
    (dict(in_src=None), b"come together"), (dict(in_dst=None), b"come together"),
    (dict(in_row_bytes=36), b"multiples of 8"), (dict(in_row_bytes=0), b"multiples of 8"), (dict(in_ld_src=44), b"multiples of 8"),
    (dict(in_ld_dst=52), b"multiples of 8"),
    (dict(in_ld_src=32), b"at least in_row_bytes"), (dict(in_ld_dst=32), b"at least in_row_bytes"),
    (dict(in_src=8196), b"8-byte aligned"), (dict(in_dst=16388), b"8-byte aligned"),
])
def test_step_begin_refuses_a_bad_job_before_any_hip_call(lib, over, text):
    rc = _begin(lib, **over)
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg and msg.startswith(b"mst_step_begin:"), (rc, msg)


def test_the_first_launch_refuses_the_same(lib):
    """mst_gemm_nt_pair_begin validates the bookkeeping it is handed the same way (the arguments of the two GEMMs are stand-ins that
    take the one-launch form, so the job's checks are what refuses the call)"""
    from musicstyletransfer_amd import _lib
    g = _lib.GemmArgs()
    for k, v in dict(dtype=_lib.MST_BF16, M=64, N=64, K=64, A=4096, lda=64, B=8192, ldb=64, C=16384, ldc=64, a_u8=1, alpha=1.0).items():
        setattr(g, k, v)
    q = _lib.StepBeginArgs()
    for k, v in dict(rng_state=4096, in_keep=4096, in_n=64, in_p=1.5, in_site=1, in_index0=0).items():
        setattr(q, k, v)
    rc = lib.mst_gemm_nt_pair_begin(ctypes.byref(g), ctypes.byref(g), ctypes.byref(q), None)
    assert rc == -1 and b"in_p" in lib.mst_last_error()


# ---------------------------------------------------------------------------------------------- the option
@pytest.mark.parametrize("bad", [-0.1, -1e-9, 1.0001, 2, float("inf"), float("-inf"), float("nan")])
def test_check_input_dropout_refuses(bad):
    from musicstyletransfer_amd import engine as E
    with pytest.raises(ValueError):
        E.check_input_dropout(bad)
    with pytest.raises(ValueError):
        _train_config(d_input_dropout=bad)


def test_check_input_dropout_accepts():
    from musicstyletransfer_amd import engine as E
    for ok in (0, 0.0, 1e-3, 0.25, 0.5, 1, 1.0):
        E.check_input_dropout(ok)
    E.check_input_dropout()
    assert "in_drop" in E.Forms._fields and E.Forms._fields[-1] == "in_drop"


def test_flag_default_and_parsing():
    from musicstyletransfer_amd.VarAutoEncoder import config, main
    a = config.get_config([])
    assert a.d_input_dropout == 0.0 and main.create_train_config(a).d_input_dropout == 0.0
    a = config.get_config(["--d-input-dropout", "0.25"])
    assert a.d_input_dropout == 0.25 and isinstance(a.d_input_dropout, float)
    assert main.create_train_config(a).d_input_dropout == 0.25  # main.py passes it through
    assert main.create_toy_train_config(3, d_input_dropout=1.0).d_input_dropout == 1.0
    with pytest.raises(SystemExit):
        config.get_config(["--d-input-dropout", "some"])
    for bad in ("-0.5", "1.5"):  # parsed, then refused where the training configuration is made
        with pytest.raises(ValueError):
            main.create_train_config(config.get_config(["--d-input-dropout", bad]))


def test_train_config_yaml_round_trip(tmp_path):
    from musicstyletransfer_amd.VarAutoEncoder import config
    tc = _train_config(d_input_dropout=0.3)
    f = str(tmp_path / "train.yaml")
    tc.save(f)
    back = config.Config.load(f)
    assert back == tc and back.d_input_dropout == 0.3 and back.kl_loss_weight == 0.5
    # a file written before the field existed: it loads with 0 (off)
    text = open(f).read().splitlines()
    lines = [ln for ln in text if not ln.startswith("d_input_dropout:")]
    assert len(lines) == len(text) - 1
    old = str(tmp_path / "old.yaml")
    open(old, "w").write("\n".join(lines) + "\n")
    back = config.Config.load(old)
    assert back.d_input_dropout == 0.0 and back == _train_config()


# ---------------------------------------------------------------------------------------------- the references
def test_masked_rows_known_answer():
    src = np.arange(1, 3 * 16 + 1, dtype=np.uint8).reshape(3, 16)
    dst = np.full((3, 24), 0xAB, np.uint8)
    out = R.masked_rows(src, [1, 0, 1], 8, dst)
    assert np.array_equal(out[0, :8], src[0, :8]) and not out[1, :8].any() and np.array_equal(out[2, :8], src[2, :8])
    assert (out[:, 8:] == 0xAB).all() and (dst == 0xAB).all()  # the rest of a row, and the argument, untouched


def test_embedding_references_against_a_loop():
    rng = np.random.default_rng(0)
    B, T, D, V, C = 2, 3, 4, 5, 2
    tok = rng.integers(0, V, (B, T))
    table, cls, pos = rng.standard_normal((V, D)), rng.standard_normal((C, D)), rng.standard_normal((T + 1, D))
    classes, keep, alpha = np.array([1, 0]), np.array([[1, 0, 1], [0, 0, 1]]), 2.0
    out = R.embed_fwd(tok, table, pos, alpha, 1, keep=keep, classes=classes, cls_table=cls)
    dX = rng.standard_normal((B, T, D))
    dtab, dcls = R.embed_bwd(tok, dX, alpha, V, keep=keep, classes=classes, n_classes=C)
    want_t, want_c = np.zeros((V, D)), np.zeros((C, D))
    for b in range(B):
        for t in range(T):
            e = table[tok[b, t]] if keep[b, t] else 0.0
            assert np.allclose(out[b, t], alpha * (e + cls[classes[b]]) + pos[1 + t], rtol=0, atol=1e-15)
            if keep[b, t]:
                want_t[tok[b, t]] += alpha * dX[b, t]
            want_c[classes[b]] += alpha * dX[b, t]
    assert np.allclose(dtab, want_t, rtol=0, atol=1e-14) and np.allclose(dcls, want_c, rtol=0, atol=1e-14)
    assert np.array_equal(R.embed_fwd(tok, table, pos, alpha, 1), R.embed_fwd(tok, table, pos, alpha, 1, keep=np.ones((B, T))))


def test_masked_decoder_installs_and_restores():
    import torch
    from oracle import vae_oracle as O
    original = O.decode_train
    cfg = O.OracleConfig("pianoroll", 8, 8, 2, 4, 8, 1, 2, 8, 1, 2)
    rng = np.random.default_rng(1)
    P = {k: torch.from_numpy(v) for k, v in O.init_params(cfg, rng).items()}
    batch = O.synthetic_pianoroll_batch(rng, 2, 3, 8, num_classes=2, density=0.3, ragged=False)
    eps = torch.from_numpy(rng.standard_normal((2, 4)).astype(np.float32))
    plain = O.model_forward(P, cfg, batch["x"], batch["seq_lens"], batch["classes"], eps)[3]
    with R.masked_decoder(np.ones((2, 3))):
        assert O.decode_train is R.decode_train
        ones = O.model_forward(P, cfg, batch["x"], batch["seq_lens"], batch["classes"], eps)[3]
    assert O.decode_train is original
    assert torch.equal(ones, plain)  # all kept: the oracle's own decoder
    with R.masked_decoder(np.zeros(6)):
        none = O.model_forward(P, cfg, batch["x"], batch["seq_lens"], batch["classes"], eps)[3]
    blank = dict(batch, x=torch.zeros_like(batch["x"]))
    means, stds = O.encode(P, cfg, batch["x"], batch["seq_lens"], batch["classes"], {})  # (the encoder sees the intact piece)
    want = O.decode_train(P, cfg, blank["x"], batch["seq_lens"], means + eps * stds, batch["classes"], {})
    assert torch.equal(none, want) and not torch.equal(none, plain)
    with pytest.raises(RuntimeError):
        with R.masked_decoder(np.ones(6)):
            raise RuntimeError("x")
    assert O.decode_train is original
