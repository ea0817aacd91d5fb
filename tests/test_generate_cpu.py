"""Latent-space generation without a GPU: the two entry points reject bad arguments before any HIP call, the recipes of every
generator mode against literal arrays, chunking, file names, the command line and the sampler names."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _rows_args(**over):
    """a valid mst_latent_rows call in ctypes terms (pointers are never followed: validation fails first in every use below)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(dtype=0, N=3, M=2, Z=16, Dd=32, zsrc=p, ssrc=None, a=p, b=p, w=p, mode=0, tau=0.0, seed=0, seed_ptr=None, site=0, row0=0,
             Wh=p, bh=p, ca=p, cb=p, cw=p, cls_d=p, ld_cls=32, n_classes=2, pos_d=p, alpha_d=1.0, z_out=p, dec_in=p, dec_stride=32, stream=None)
    a.update(over)
    a["_keep"] = buf
    return a


def _rows(lib, **over):
    a = _rows_args(**over)
    a.pop("_keep")
    return lib.mst_latent_rows(*a.values())


@pytest.mark.parametrize("over,text", [
    (dict(zsrc=None), b"null source"), (dict(a=None), b"null source"), (dict(w=None), b"null source"),
    (dict(ca=None), b"class index"), (dict(cb=None), b"class index"), (dict(cw=None), b"class index"),
    (dict(Wh=None), b"null pointer"), (dict(z_out=None), b"null pointer"), (dict(dec_in=None), b"null pointer"),
    (dict(tau=-0.5), b"tau < 0"), (dict(mode=2), b"mode"), (dict(N=0), b"sizes"), (dict(row0=-1), b"sizes"),
    (dict(n_classes=0), b"class table"), (dict(dec_stride=16), b"class table"), (dict(dtype=7), b"unsupported activation dtype"),
])
def test_latent_rows_rejects_bad_arguments(lib, over, text):
    rc = _rows(lib, **over)
    assert rc != 0 and text in lib.mst_last_error(), (rc, lib.mst_last_error())
    if "dtype" not in over:
        assert rc == -1


def _frame(lib, **over):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(dtype=0, N=4, P=8, i=1, L=4, logits=p, ldl=8, tau=1.0, mode=0, thr=0.5, seed_ptr=p, frames=p, ldf=8, roll=p, ldr=8, scores=p,
             probs_out=None, stream=None)
    a.update(over)
    return lib.mst_frame_step(*a.values())


@pytest.mark.parametrize("over,text", [
    (dict(logits=None), b"null pointer"), (dict(frames=None), b"null pointer"), (dict(roll=None), b"null pointer"),
    (dict(scores=None), b"null pointer"), (dict(seed_ptr=None), b"seed word"),
    (dict(mode=1, thr=0.0), b"thr outside"), (dict(mode=1, thr=1.0), b"thr outside"), (dict(mode=1, thr=-0.2), b"thr outside"),
    (dict(tau=-1.0), b"tau"), (dict(tau=0.0), b"tau"), (dict(i=0), b"outside [1, L)"), (dict(i=4), b"outside [1, L)"),
    (dict(mode=3), b"mode"), (dict(ldf=4), b"stride"),
])
def test_frame_step_rejects_bad_arguments(lib, over, text):
    rc = _frame(lib, **over)
    assert rc == -1 and text in lib.mst_last_error(), (rc, lib.mst_last_error())


def test_wrappers_raise_with_the_library_message(lib):
    from musicstyletransfer_amd import _lib
    with pytest.raises(_lib.MstError, match="class index"):
        a = _rows_args(ca=None)
        a.pop("_keep")
        _lib.call("mst_latent_rows", *a.values())


# ---------------------------------------------------------------------- recipes
def test_prior_recipe():
    from musicstyletransfer_amd import generate as G
    r = G.recipe_prior(5, [0, 1, 2, 0, 1], temperature=0.7)
    assert r.a.dtype == np.int32 and r.w.dtype == np.float32
    assert r.a.tolist() == [-1] * 5 and r.b.tolist() == [-1] * 5 and r.w.tolist() == [0.0] * 5
    assert r.ca.tolist() == [0, 1, 2, 0, 1] and r.cb.tolist() == [0, 1, 2, 0, 1] and r.cw.tolist() == [0.0] * 5
    assert r.tau == 0.7 and not r.use_sigma
    assert r.files == ["prior-0.class-0.mid", "prior-1.class-1.mid", "prior-2.class-2.mid", "prior-3.class-0.mid", "prior-4.class-1.mid"]
    assert r.rows[3] == dict(n=3, cls=0)
    assert G.recipe_prior(3, 2).ca.tolist() == [2, 2, 2]      # one class for every row
    r.validate(0, 3)                                           # a prior recipe needs no source vectors
    with pytest.raises(ValueError):
        r.validate(0, 2)                                       # class 2 of a two-class model
    with pytest.raises(ValueError):
        G.recipe_prior(4, [0, 1])


def test_posterior_recipe():
    from musicstyletransfer_amd import generate as G
    r = G.recipe_posterior([1, 0, 2], 2, temperature=1.5)
    assert r.a.tolist() == [0, 0, 1, 1, 2, 2] and r.b.tolist() == r.a.tolist() and r.w.tolist() == [0.0] * 6
    assert r.ca.tolist() == [1, 1, 0, 0, 2, 2] and r.cb.tolist() == r.ca.tolist()
    assert r.tau == 1.5 and r.use_sigma and r.mode == "lerp"
    assert r.files == ["posterior-0.draw-0.mid", "posterior-0.draw-1.mid", "posterior-1.draw-0.mid", "posterior-1.draw-1.mid",
                       "posterior-2.draw-0.mid", "posterior-2.draw-1.mid"]
    with pytest.raises(ValueError):
        r.validate(2, 3)                                       # melody 2 of a two-melody encode


def test_interpolation_recipe():
    from musicstyletransfer_amd import generate as G
    r = G.recipe_interpolate(2, 0, 7, class_i=1, class_j=0)
    assert r.a.tolist() == [2] * 7 and r.b.tolist() == [0] * 7
    np.testing.assert_array_equal(r.w, np.array([0, 1 / 6, 2 / 6, 3 / 6, 4 / 6, 5 / 6, 1], np.float32))
    assert r.w[0] == 0.0 and r.w[-1] == 1.0                   # the end points are the sources themselves
    assert r.ca.tolist() == [1, 1, 1, 1, 0, 0, 0] and r.cb.tolist() == r.ca.tolist() and r.cw.tolist() == [0.0] * 7
    assert r.mode == "slerp" and r.tau == 0.0
    assert r.files[0] == "interp-2-0.00.mid" and r.files[6] == "interp-2-0.06.mid" and len(set(r.files)) == 7
    assert G.recipe_interpolate(0, 1, 4, 0, 1).ca.tolist() == [0, 0, 1, 1]
    assert G.recipe_interpolate(0, 1, 3, 0, 1, classes=[1, 1, 0], mode="lerp").ca.tolist() == [1, 1, 0]
    with pytest.raises(ValueError):
        G.recipe_interpolate(0, 1, 1, 0, 1)
    with pytest.raises(ValueError):
        G.recipe_interpolate(0, 1, 3, 0, 1, mode="cubic")


def test_transfer_and_blend_recipes():
    from musicstyletransfer_amd import generate as G
    r = G.recipe_transfer(2, [0, 1, 2])
    assert r.a.tolist() == [0, 0, 0, 1, 1, 1] and r.b.tolist() == r.a.tolist()
    assert r.ca.tolist() == [0, 1, 2, 0, 1, 2] and r.cb.tolist() == r.ca.tolist()
    assert r.w.tolist() == [0.0] * 6 and r.cw.tolist() == [0.0] * 6 and r.tau == 0.0
    assert r.files == ["transfer-0.class-0.mid", "transfer-0.class-1.mid", "transfer-0.class-2.mid", "transfer-1.class-0.mid",
                       "transfer-1.class-1.mid", "transfer-1.class-2.mid"]
    assert r.rows[4] == dict(melody=1, cls=1)
    b = G.recipe_class_blend(2, 2, 0, [0.0, 0.25, 1.0])
    assert b.a.tolist() == [0, 0, 0, 1, 1, 1] and b.ca.tolist() == [2] * 6 and b.cb.tolist() == [0] * 6
    np.testing.assert_array_equal(b.cw, np.array([0, 0.25, 1, 0, 0.25, 1], np.float32))
    assert b.files[1] == "blend-0.class-2-0.01.mid" and b.files[5] == "blend-1.class-2-0.02.mid"
    assert b.rows[1]["weight"] == 0.25 and b.rows[1]["melody"] == 0


def test_chunking_at_max_rows():
    from musicstyletransfer_amd import generate as G
    assert G.chunks(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert G.chunks(8, 4) == [(0, 4), (4, 8)] and G.chunks(3, 256) == [(0, 3)]
    with pytest.raises(ValueError):
        G.chunks(3, 0)
    with pytest.raises(ValueError):
        G.LatentGenerator(None, decoder="nucleus")
    with pytest.raises(ValueError):
        G.LatentGenerator(None, max_rows=0)


def test_command_line_parser():
    from music_style_transfer.VarAutoEncoder import generate as G
    from musicstyletransfer_amd import generate as impl
    assert G.LatentGenerator is impl.LatentGenerator                      # the reference's package name reaches the same module
    p = G.build_parser()
    a = p.parse_args(["--model-output", "m", "--mode", "interpolate", "--toy", "--steps", "5", "--temperature", "0.5", "--decoder", "greedy",
                      "--seed", "7", "--out", "o"])
    assert (a.model_output, a.mode, a.toy, a.steps, a.temperature, a.decoder, a.seed, a.out, a.checkpoint) == \
        ("m", "interpolate", True, 5, 0.5, "greedy", 7, "o", -1)
    a = p.parse_args(["--model-output", "m", "--checkpoint", "3", "--mode", "prior", "--n", "6", "--out", "o", "--data", "d"])
    assert a.checkpoint == 3 and a.n == 6 and a.data == "d" and not a.toy
    for bad in (["--model-output", "m", "--mode", "nucleus", "--out", "o"], ["--mode", "prior", "--out", "o"],
                ["--model-output", "m", "--mode", "prior", "--out", "o", "--toy", "--data", "d"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_the_module_runs_under_the_reference_package_name():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "music_style_transfer.VarAutoEncoder.generate", "--help"], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0 and "--mode" in r.stdout and "--model-output" in r.stdout, r.stderr


def test_sampler_names():
    from music_style_transfer.VarAutoEncoder import sampler as S

    class A:
        verbose, beam_size = False, 3

    for name, cls in (("prior", S.PriorSampler), ("interpolation", S.InterpolationSampler), ("transfer", S.TransferSampler)):
        assert type(S.get_sampler(name, None, None, None, A)) is cls
    assert type(S.get_sampler("sampling", None, None, None, A)) is S.Sampling
    assert S.Sampling().frames_on_device is False and S.Sampling(frames_on_device=True).frames_on_device is True
    for name in ("nucleus", "top-k", ""):
        with pytest.raises(ValueError):
            S.get_sampler(name, None, None, None, A)
