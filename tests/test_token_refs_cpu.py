"""mst_token_step without a GPU: the fp64 references of its cuts against each other and against the properties the header states,
the case generator's margin, and the entry point's argument checks (which run before any HIP call)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_refs as T  # noqa: E402

_DT = {torch.bfloat16: "bf16", torch.float16: "fp16"}
CPU_V = tuple(v for v in T.SAMPLE_V if v > 1)


@pytest.mark.parametrize("dtype", T.DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("V", T.SAMPLE_V, ids=lambda v: f"V{v}")
def test_cut_form_equals_the_brute_force_form(V, dtype):
    for tau in T.TAUS:
        for ties in (False, True):
            row = T.make_row(V, dtype, seed=V)
            if ties:
                row = T.plant_ties(row, 7)
            for top_k in (0, 1, 2, 7, V - 1, V, V + 5):
                if top_k < 0:
                    continue
                for top_p in (1.0, 0.95, 0.5, 0.07, 1e-6):
                    kept, s, p = T.token_filter_ref(row, tau, top_k, top_p)
                    brute = T.token_filter_brute(row, tau, top_k, top_p)
                    assert np.array_equal(kept, brute), (V, tau, ties, top_k, top_p)
                    assert kept[int(np.argmax(row.double().numpy()))]          # the arg-max is always kept
                    assert abs(s.sum() - 1) < 1e-12 and abs(p.sum() - 1) < 1e-12
                    v = row.double().numpy()
                    assert v[kept].min() > v[~kept].max() if (~kept).any() else True  # a cut on the value: no tie group is split


@pytest.mark.parametrize("dtype", T.DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("V", CPU_V, ids=lambda v: f"V{v}")
def test_the_generators_margin_holds(V, dtype):
    """every target has a step wider than 4 delta, for every temperature and top-k the GPU tests use; top_p then sits at least
    2 delta from both neighbouring cumulative masses, and the reference keeps exactly the values down to that step"""
    row = T.make_row(V, dtype, seed=V)
    for tau in T.TAUS:
        for top_k in (0, 7):
            for target in T.TARGETS:
                top_p, n_vals = T.fit_top_p(row, tau, top_k, target)
                assert 0.0 < top_p < 1.0 and float(np.float32(top_p)) == top_p
                assert T.margin(row, tau, top_k, top_p) >= 2.0, (V, tau, top_k, target, top_p)
                kept, _, _ = T.token_filter_ref(row, tau, top_k, top_p)
                assert len(np.unique(row.double().numpy()[kept])) == n_vals


def test_filters_off_keep_all_and_top_1_keeps_the_argmax_group():
    for V in T.SAMPLE_V:
        row = T.make_row(V, torch.bfloat16, seed=3 * V)
        kept, _, _ = T.token_filter_ref(row, 0.7, 0, 1.0)
        assert kept.all()
        assert T.token_filter_ref(row, 0.7, V, 1.0)[0].all() and T.token_filter_ref(row, 0.7, V + 1, 1.0)[0].all()
        one, _, _ = T.token_filter_ref(row, 0.7, 1, 1.0)
        v = row.double().numpy()
        assert np.array_equal(one, v == v.max())
    row = torch.tensor([0.5, 2.0, -1.0, 2.0, 0.25], dtype=torch.float16)
    assert T.token_filter_ref(row, 1.0, 1, 1.0)[0].tolist() == [False, True, False, True, False]
    assert T.token_filter_ref(row, 1.0, 0, 1e-6)[0].tolist() == [False, True, False, True, False]  # the smallest nucleus: the same group


def test_a_tie_group_straddling_k_is_kept_whole():
    row = T.plant_ties(T.make_row(64, torch.bfloat16, seed=11), 7)
    v = row.double().numpy()
    ck = np.sort(v)[::-1][6]
    assert (v == ck).sum() == 9 and (v > ck).sum() == 2       # ranks 3..11 hold one value: k = 7 falls inside the group
    kept, _, _ = T.token_filter_ref(row, 1.0, 7, 1.0)
    assert kept.sum() == 11 and np.array_equal(kept, v >= ck)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1))
    kept_perm, _, _ = T.token_filter_ref(row[perm], 1.0, 7, 1.0)
    assert np.array_equal(kept_perm, kept[perm.numpy()])       # a function of the values, not of the column order


def test_kept_sets_nest_as_top_p_falls():
    for V in (5, 65, 293):
        for dtype in T.DTYPES:
            row = T.make_row(V, dtype, seed=V + 1)
            for top_k in (0, 7):
                prev = T.token_filter_ref(row, 1.3, top_k, 1.0)[0]
                for top_p in (0.99, 0.9, 0.7, 0.5, 0.3, 0.1, 0.01):
                    kept = T.token_filter_ref(row, 1.3, top_k, top_p)[0]
                    assert (prev | ~kept).all() and kept.any(), (V, top_k, top_p)
                    prev = kept


# ---------------------------------------------------------------------- the entry point's argument checks
@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _token(lib, **over):
    """a valid mst_token_step call in ctypes terms (pointers are never followed: validation fails first in every use below)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(dtype=0, N=4, V=8, i=1, L=4, logits=p, ldl=8, tau=1.0, top_k=0, top_p=1.0, seed_ptr=p, seqs=p, scores=p, word=p, active=None,
             kept_out=None, eos=2, pad=0, stream=None)
    a.update(over)
    return lib.mst_token_step(*a.values())


@pytest.mark.parametrize("over,text", [
    (dict(tau=0.0), b"tau"), (dict(tau=-1.0), b"tau"), (dict(tau=float("inf")), b"tau"), (dict(tau=float("nan")), b"tau"),
    (dict(top_k=-1), b"top_k"), (dict(top_p=0.0), b"top_p outside"), (dict(top_p=-0.5), b"top_p outside"),
    (dict(top_p=1.5), b"top_p outside"), (dict(top_p=float("nan")), b"top_p outside"),
    (dict(i=0), b"outside [1, L)"), (dict(i=4), b"outside [1, L)"), (dict(ldl=7), b"stride"),
    (dict(logits=None), b"null pointer"), (dict(seed_ptr=None), b"null pointer"), (dict(seqs=None), b"null pointer"),
    (dict(scores=None), b"null pointer"), (dict(word=None), b"null pointer"), (dict(N=0), b"sizes"), (dict(V=0), b"sizes"),
])
def test_token_step_rejects_bad_arguments(lib, over, text):
    rc = _token(lib, **over)
    assert rc == -1 and text in lib.mst_last_error(), (rc, lib.mst_last_error())


def test_token_step_is_abi_102(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 102
    assert len(_lib.SIGNATURES["mst_token_step"][1]) == 19 and len(_lib.STRUCTS) == 12
    assert _token(lib, dtype=7) != 0 and b"unsupported activation dtype" in lib.mst_last_error()


# ---------------------------------------------------------------------- the public interface, as far as it goes without a GPU
def test_command_line_and_constructors_take_the_draws_settings():
    from music_style_transfer.VarAutoEncoder import generate as G, sampler as S
    p = G.build_parser()
    a = p.parse_args(["--model-output", "m", "--mode", "prior", "--out", "o"])
    assert (a.sample_temperature, a.top_k, a.top_p) == (1.0, 0, 1.0)
    a = p.parse_args(["--model-output", "m", "--mode", "prior", "--out", "o", "--sample-temperature", "0.8", "--top-k", "40", "--top-p", "0.9"])
    assert (a.sample_temperature, a.top_k, a.top_p) == (0.8, 40, 0.9)
    g = G.LatentGenerator(None, sample_temperature=0.8, top_k=40, top_p=0.9)
    assert (g.sample_temperature, g.top_k, g.top_p, g.frame_temperature) == (0.8, 40, 0.9, 0.8)
    g = G.LatentGenerator(None)
    assert (g.sample_temperature, g.top_k, g.top_p, g.frame_temperature) == (1.0, 0, 1.0, 1.0)
    assert G.LatentGenerator(None, frame_temperature=0.5).frame_temperature == 0.5   # the earlier keyword keeps working
    for decoder in ("beam", "greedy"):
        for kw in (dict(top_k=3), dict(top_p=0.5)):
            with pytest.raises(ValueError):
                G.LatentGenerator(None, decoder=decoder, **kw)
    for kw in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.01), dict(sample_temperature=0.0), dict(sample_temperature=float("inf")),
               dict(sample_temperature=0.5, frame_temperature=0.7)):
        with pytest.raises(ValueError):
            G.LatentGenerator(None, **kw)
    s = S.Sampling(temperature=0.7, top_k=5, top_p=0.9)
    assert (s.temperature, s.top_k, s.top_p) == (0.7, 5, 0.9) and S.Sampling().top_k == 0
    for kw in (dict(temperature=0.0), dict(top_k=-2), dict(top_p=0.0)):
        with pytest.raises(ValueError):
            S.Sampling(**kw)

    class A:
        verbose, beam_size, sample_temperature, top_k, top_p = False, 3, 0.9, 7, 0.8

    t = S.get_sampler("transfer", None, None, None, A)
    assert (t.sample_temperature, t.top_k, t.top_p) == (0.9, 7, 0.8)
    smp = S.get_sampler("sampling", None, None, None, A)
    assert (smp.temperature, smp.top_k, smp.top_p) == (0.9, 7, 0.8)
