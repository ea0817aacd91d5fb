"""The references and input generators the decode-kernel GPU tests rely on (tests/decode_refs.py), checked where no GPU is needed:
the vectorised beam_step_ref against a brute-force loop, the generators against the gaps and ties they promise for every size the GPU
tests run, the attention bound against the rounded reference, the recorded storage cost of the long decode against a fresh measurement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_refs as R  # noqa: E402


def test_token_ids_are_the_librarys():
    from musicstyletransfer_amd.MIDIUtil import defaults as d
    assert (R.EOS, R.PAD, R.SOS) == (d.EOS_ID, d.PAD_ID, d.SOS_ID) and d.NUM_EVENTS == 293


def _same(a, b):
    for k in ("seqs", "hyp_src", "word"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["scores"], b["scores"]) and a["alive"] == b["alive"]  # (the same fp64 operations: bit for bit)


@pytest.mark.parametrize("K,V", [(1, 5), (3, 4), (4, 3), (5, 1), (2, 7)])
@pytest.mark.parametrize("i", [1, 2, 4])
def test_beam_step_ref_against_a_brute_force_loop(K, V, i):
    B, L = 4, 6
    rng = np.random.default_rng(10 * K + V + i)
    for variant in ("random", "ties", "finished", "nonfinite", "first"):
        if variant in ("ties", "first"):
            probs, scores, seqs = R.beam_tie_case(B, K, V, 1 if variant == "first" else i, seed=K + V, L=L, first_position=variant == "first")
            pos = 1 if variant == "first" else i
        else:
            pos = i
            last = rng.choice(np.array([R.EOS, R.PAD, 9], np.int32), size=B * K) if variant == "finished" else None
            probs, scores, seqs = R.beam_separated_case(B, K, V, i, seed=K * V + i, L=L, last=last)
            if variant == "nonfinite":
                probs[0, 0] = np.nan
                scores[B * K - 1] = np.nan
                probs[1 % (B * K), V - 1] = 0.0
        _same(R.beam_step_ref(probs, scores, seqs, pos, K), R.beam_step_bruteforce(probs, scores, seqs, pos, K))


def test_beam_step_ref_on_a_case_worked_by_hand():
    """K = 2, V = 3, i = 2: hypothesis 0 is live at score 1 with p = (.5, .25, .25), hypothesis 1 ended in EOS at score 1.5"""
    probs = np.array([[0.5, 0.25, 0.25], [0.1, 0.8, 0.1]], np.float32)
    seqs = np.array([[1, 7, 0], [1, R.EOS, 0]], np.int32)
    ref = R.beam_step_ref(probs, np.array([1.0, 1.5], np.float32), seqs, 2, 2)
    # candidates: 1 + ln 2 = 1.693 (0, PAD), 1 + ln 4 = 2.386 twice, 1.5 (1, PAD), inf, inf
    assert ref["hyp_src"].tolist() == [1, 0] and ref["word"].tolist() == [R.PAD, R.PAD]
    assert ref["seqs"].tolist() == [[1, R.EOS, R.PAD], [1, 7, R.PAD]]
    np.testing.assert_allclose(ref["scores"], [1.5, 1.0 + np.log(2.0)], rtol=1e-15)
    assert ref["alive"] == 0
    # position 1: a PAD in column 0 does not finish a hypothesis
    seqs1 = np.array([[R.PAD, 0, 0], [R.EOS, 0, 0]], np.int32)
    ref = R.beam_step_ref(probs, np.array([1.0, 1.5], np.float32), seqs1, 1, 2)
    assert ref["hyp_src"].tolist() == [1, 0] and ref["word"].tolist() == [R.PAD, R.PAD] and ref["scores"][1] == 1.0 + np.log(2.0)
    seqs1[1, 0] = 9
    ref = R.beam_step_ref(probs, np.array([1.0, 1.5], np.float32), seqs1, 1, 2)
    assert ref["hyp_src"].tolist() == [0, 1] and ref["word"].tolist() == [0, 1] and ref["alive"] == 1  # 1.693 < 1.5 - ln .8 = 1.723


@pytest.mark.parametrize("pos", [1, 2, R.BEAM_L - 1])
@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("K,V", R.BEAM_SIZES, ids=lambda v: str(v))
def test_the_separated_generator_produces_the_gap_for_every_sample(K, V, B, pos):
    """the seeds of test_beam_step_is_the_stable_argsort: no sample is left under the gap, none is dropped"""
    probs, scores, seqs = R.beam_separated_case(B, K, V, pos, seed=100 * K + V + pos)
    gap = R.beam_min_gap(probs, scores, seqs, pos, K)
    assert gap.shape == (B,) and (gap >= R.REL_GAP).all()
    assert probs.shape == (B * K, V) and np.isfinite(probs).all() and (probs > 0).all() and (scores >= 0).all()
    # and the gap is what it says: the reference's best 2 K, sorted, differ pairwise by REL_GAP (relative)
    top = np.sort(R.beam_scores(probs, scores, seqs, pos, K), axis=1)[:, :2 * K]
    assert (np.diff(top, axis=1) >= R.REL_GAP * np.abs(top[:, 1:]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("K,V", R.BEAM_SIZES, ids=lambda v: str(v))
def test_the_tie_generator_produces_exact_ties(K, V, first):
    i = 1 if first else 3
    probs, scores, seqs = R.beam_tie_case(5, K, V, i, seed=7 * K + V, first_position=first)
    assert R.beam_ties_are_exact(probs, scores, seqs, i, K)
    if K > 1:
        assert np.array_equal(probs[0], probs[1]) and (first or scores[0] == scores[1])
    top = np.sort(R.beam_scores(probs, scores, seqs, i, K), axis=1)[:, :K + 1]
    if K * V >= 64:  # enough candidates over six levels: the selection does cut through a group of equal scores
        assert (top[:, :-1] == top[:, 1:]).any()


@pytest.mark.parametrize("n_keys", R.ATTN_NKEYS)
@pytest.mark.parametrize("mode,kind", [(0, "random"), (1, "random"), (1, "dominant"), (1, "uniform")])
@pytest.mark.parametrize("dtype", R.ATTN_DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("dh", R.ATTN_DH)
def test_the_attention_bound_holds_for_the_rounded_reference(dh, dtype, mode, kind, n_keys):
    """the fp64 answer rounded once to the output type is inside attn_decode_tol; the generator's cache is NaN wherever the kernel has
    no business reading; the 'dominant' and 'uniform' kinds carry logits beyond 100"""
    B, H = 3, 2
    D = H * dh
    cache, (ld, k_off, q_off, v_off) = R.attn_case(B, H, dh, n_keys, dtype, mode, seed=1000 * dh + 10 * n_keys + mode, kind=kind)
    ref = R.attn_decode_ref(cache, n_keys, H, dh, k_off, q_off, v_off, mode)
    tol = R.attn_decode_tol(ref, cache, n_keys, H, dh, v_off, mode)
    assert torch.isfinite(ref).all() and ((ref.to(dtype).double() - ref).abs() <= tol).all()
    finite = torch.isfinite(cache)
    assert finite[:, :n_keys, k_off:k_off + D].all() and finite[:, :n_keys, v_off:v_off + D].all() and finite[:, n_keys - 1, q_off:q_off + D].all()
    assert int(finite.sum()) == B * (2 * n_keys + 1) * D
    lg = R.attn_logits(cache, n_keys, H, dh, k_off, q_off, v_off).abs().max()
    assert float(lg) > 100.0 if kind != "random" else float(lg) < 20.0


def test_attention_reference_on_known_answers():
    for dtype in R.ATTN_DTYPES:
        cache, (ld, k_off, q_off, v_off) = R.attn_case(2, 2, 16, 65, dtype, 1, seed=1, layout=R.SPREAD, kind="uniform")
        _, V, _ = R.attn_parts(cache, 65, 2, 16, k_off, q_off, v_off)
        ref = R.attn_decode_ref(cache, 65, 2, 16, k_off, q_off, v_off, 1)
        np.testing.assert_allclose(ref.numpy(), V.mean(1).reshape(2, -1).numpy(), rtol=1e-12, atol=1e-14)
        cache, (ld, k_off, q_off, v_off) = R.attn_case(2, 2, 16, 65, dtype, 1, seed=2, kind="dominant")
        _, V, _ = R.attn_parts(cache, 65, 2, 16, k_off, q_off, v_off)
        lg = R.attn_logits(cache, 65, 2, 16, k_off, q_off, v_off)
        assert (lg.argmax(-1) == 32).all() and float((lg.amax(-1, keepdim=True) - lg).topk(2, largest=False).values[..., 1].min()) > 55.0
        np.testing.assert_allclose(R.attn_decode_ref(cache, 65, 2, 16, k_off, q_off, v_off, 1).numpy(), V[:, 32].reshape(2, -1).numpy(), atol=1e-20)
        assert torch.equal(R.attn_decode_ref(cache, 65, 2, 16, k_off, q_off, v_off, 0), V.sum(1).reshape(2, -1))


@pytest.mark.parametrize("attention", ["query", "key"])
@pytest.mark.parametrize("kind", ["token", "pianoroll"])
def test_the_recorded_storage_cost_is_what_the_oracle_measures(kind, attention):
    """test_long_decode_matches_the_oracle's bound is twice these figures; they are re-measured here (to the three digits recorded)"""
    np.testing.assert_allclose(R.storage_cost(kind, attention), R.STORAGE_COST[(kind, attention)], rtol=1e-2)
