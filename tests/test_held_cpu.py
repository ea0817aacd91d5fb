"""Constrained decoding without a GPU: both held entry points refuse bad arguments before any HIP call, hold_mask on ragged lengths,
the piece of a token batch, what continue_ hands the encoder, beam search refusing a constraint, the three command-line modes, and
the fp64 references of tests/held_refs.py against a direct per-cell loop."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_refs as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _frame(lib, **over):
    """a valid mst_frame_step_held call in ctypes terms (pointers are never followed: validation fails first in every use below)"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(dtype=0, N=4, P=8, i=1, L=4, logits=p, ldl=8, tau=1.0, mode=0, thr=0.5, seed_ptr=p, frames=p, ldf=8, roll=p, ldr=8, scores=p,
             probs_out=None, given=p, ldg=8, hold=p, ldh=8, held_scores=p, stream=None)
    a.update(over)
    return lib.mst_frame_step_held(*a.values())


def _token(lib, **over):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(dtype=0, N=4, V=8, i=1, L=4, logits=p, ldl=8, tau=1.0, top_k=0, top_p=1.0, seed_ptr=p, seqs=p, scores=p, word=p, active=None,
             kept_out=None, eos=2, pad=0, given=p, hold=p, held_scores=p, stream=None)
    a.update(over)
    return lib.mst_token_step_held(*a.values())


def test_the_abi_has_the_two_entry_points(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 117
    assert len(_lib.SIGNATURES["mst_frame_step_held"][1]) == len(_lib.SIGNATURES["mst_frame_step"][1]) + 5
    assert len(_lib.SIGNATURES["mst_token_step_held"][1]) == len(_lib.SIGNATURES["mst_token_step"][1]) + 3
    # the new arguments sit between the old ones and the stream
    assert _lib.SIGNATURES["mst_frame_step_held"][1][:17] == _lib.SIGNATURES["mst_frame_step"][1][:17]
    assert _lib.SIGNATURES["mst_token_step_held"][1][:18] == _lib.SIGNATURES["mst_token_step"][1][:18]


@pytest.mark.parametrize("over,text", [
    (dict(given=None), b"given, hold, held_scores"), (dict(hold=None), b"given, hold, held_scores"),
    (dict(held_scores=None), b"given, hold, held_scores"), (dict(ldg=7), b"stride below P"), (dict(ldh=4), b"stride below P"),
    (dict(ldf=4), b"stride below P"), (dict(ldl=7), b"stride below P"), (dict(ldr=0), b"stride below P"),
    (dict(logits=None), b"null pointer"), (dict(frames=None), b"null pointer"), (dict(roll=None), b"null pointer"),
    (dict(scores=None), b"null pointer"), (dict(seed_ptr=None), b"seed word"),
    (dict(i=0), b"outside [1, L)"), (dict(i=4), b"outside [1, L)"), (dict(i=-1), b"outside [1, L)"),
    (dict(tau=0.0), b"tau"), (dict(tau=-1.0), b"tau"), (dict(tau=float("inf")), b"tau"), (dict(tau=float("nan")), b"tau"),
    (dict(mode=2), b"mode"), (dict(mode=1, thr=1.0), b"thr outside"), (dict(N=0), b"sizes"), (dict(L=1, i=1), b"sizes"),
])
def test_frame_step_held_rejects_bad_arguments(lib, over, text):
    rc = _frame(lib, **over)
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg and msg.startswith(b"mst_frame_step_held:"), (rc, msg)


@pytest.mark.parametrize("over,text", [
    (dict(given=None), b"given, hold, held_scores"), (dict(hold=None), b"given, hold, held_scores"),
    (dict(held_scores=None), b"given, hold, held_scores"),
    (dict(logits=None), b"null pointer"), (dict(seed_ptr=None), b"null pointer"), (dict(seqs=None), b"null pointer"),
    (dict(scores=None), b"null pointer"), (dict(word=None), b"null pointer"),
    (dict(i=0), b"outside [1, L)"), (dict(i=4), b"outside [1, L)"), (dict(ldl=7), b"stride"),
    (dict(tau=0.0), b"tau"), (dict(tau=-1.0), b"tau"), (dict(tau=float("inf")), b"tau"), (dict(tau=float("nan")), b"tau"),
    (dict(top_k=-1), b"top_k"), (dict(top_p=0.0), b"top_p outside"), (dict(top_p=1.5), b"top_p outside"),
    (dict(N=0), b"sizes"), (dict(V=0), b"sizes"),
])
def test_token_step_held_rejects_bad_arguments(lib, over, text):
    rc = _token(lib, **over)
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg and msg.startswith(b"mst_token_step_held:"), (rc, msg)


def test_bad_dtype_is_refused_and_the_old_entry_points_keep_their_names(lib):
    assert _frame(lib, dtype=7) != 0 and b"unsupported activation dtype" in lib.mst_last_error()
    assert _token(lib, dtype=7) != 0 and b"unsupported activation dtype" in lib.mst_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mst_frame_step(0, 4, 8, 0, 4, p, 8, 1.0, 0, 0.5, p, p, 8, p, 8, p, None, None) == -1
    assert lib.mst_last_error().startswith(b"mst_frame_step: position i")
    assert lib.mst_token_step(0, 4, 8, 0, 4, p, 8, 1.0, 0, 1.0, p, p, p, p, None, None, 2, 0, None) == -1
    assert lib.mst_last_error().startswith(b"mst_token_step: position i")


# ---------------------------------------------------------------------- hold_mask and the pieces
def test_hold_mask_on_ragged_lengths():
    from musicstyletransfer_amd import generate as G
    lens, T, P = np.array([5, 2, 0, 7]), 6, 4
    t, j = np.arange(T), np.arange(P)
    inside = t[None, :] < lens[:, None]
    m = G.hold_mask(lens, T, P)
    assert m.dtype == bool and m.shape == (4, T, P) and np.array_equal(m, np.broadcast_to(inside[:, :, None], m.shape))
    m = G.hold_mask(lens, T, P, time=(1, 4))
    assert np.array_equal(m, np.broadcast_to((inside & ((t >= 1) & (t < 4)))[:, :, None], m.shape))
    m = G.hold_mask(lens, T, P, pitch=(1, 3))
    assert np.array_equal(m, inside[:, :, None] & ((j >= 1) & (j < 3))[None, None, :])
    m = G.hold_mask(lens, T, P, time=(0, 3), pitch=(2, 9))
    assert np.array_equal(m, (inside & (t < 3))[:, :, None] & (j >= 2)[None, None, :])
    assert m[0, 2, 3] and not m[0, 3, 3] and not m[0, 2, 1] and not m[1, 2, 3] and not m[2].any()
    for kw in (dict(time=(3, 3)), dict(time=(4, 2)), dict(pitch=(2, 2)), dict(time=(6, 9)), dict(pitch=(4, 8))):
        assert not G.hold_mask(lens, T, P, **kw).any(), kw
    for kw in (dict(), dict(time=(0, 99)), dict(pitch=(0, 99)), dict(time=(2, 5), pitch=(1, 2))):
        m = G.hold_mask(lens, T, P, **kw)
        for b, n in enumerate(lens):
            assert not m[b, n:].any(), (kw, b)  # never at or behind a row's length
    m = G.hold_mask(lens, T)  # token ends: no pitch axis
    assert m.shape == (4, T) and np.array_equal(m, inside)
    assert np.array_equal(G.hold_mask(lens, T, time=(1, 3)), inside & ((t >= 1) & (t < 3)))
    with pytest.raises(ValueError):
        G.hold_mask(lens, T, pitch=(0, 2))
    with pytest.raises(ValueError):
        G.hold_mask(lens, 0)


def test_the_token_piece_carries_its_eos():
    from musicstyletransfer_amd import generate as G
    from musicstyletransfer_amd.VarAutoEncoder.data import ToyData
    toy = ToyData()
    piece = G.token_piece(toy.tokens, toy.seq_lens)
    # position i is fed tokens[i - 1] and scored against labels[i - 1] in training: the piece is SOS followed by the labels
    assert np.array_equal(piece[:, 0], toy.tokens[:, 0]) and np.array_equal(piece[:, 1:], toy.labels)
    ragged = G.token_piece([[1, 5, 6, 7, 9], [1, 6, 0, 0, 0]], [5, 2])
    assert ragged.tolist() == [[1, 5, 6, 7, 9, 2], [1, 6, 2, 0, 0, 0]]


class _Encoder:
    """stands where the model stands in LatentGenerator: records what continue_ hands the encoder and stops there"""

    class Stop(Exception):
        pass

    def encode(self, x, lens, classes):
        self.x, self.lens, self.classes = np.asarray(x), np.asarray(lens), np.asarray(classes)
        raise self.Stop


def test_continue_encodes_the_opening_only():
    from musicstyletransfer_amd import generate as G
    from musicstyletransfer_amd.VarAutoEncoder.data import Batch
    rng = np.random.default_rng(0)
    B, T, P = 4, 9, 6
    labels = (rng.random((B, T, P)) < 0.3).astype(np.uint8)
    x = np.zeros_like(labels)
    x[:, 0, 0] = 1
    x[:, 1:] = labels[:, :-1]
    lens = np.array([9, 2, 5, 3])
    enc = _Encoder()
    gen = G.LatentGenerator(None, decoder="greedy")
    gen.model = enc
    with pytest.raises(_Encoder.Stop):
        gen.continue_(Batch([x, lens, np.array([0, 1, 0, 1])], [labels]), prime=3)
    assert enc.lens.tolist() == [3, 2, 3, 3]
    assert np.array_equal(enc.x[:, :3], x[:, :3]) and not enc.x[:, 3:].any() and x[:, 3:].any()  # (and the batch itself is untouched)
    x_o, l_o = G.opening(np.array([[1, 5, 6, 7, 0]]), [4], 2)
    assert x_o.tolist() == [[1, 5, 0, 0, 0]] and l_o.tolist() == [2]
    with pytest.raises(ValueError):
        G.opening(x, lens, 0)


def test_recipes_of_the_constrained_modes():
    from musicstyletransfer_amd import generate as G
    r = G.recipe_continue([1, 0, 2], 2)
    assert r.a.tolist() == [0, 0, 1, 1, 2, 2] and r.ca.tolist() == [1, 1, 0, 0, 2, 2] and r.tau == 0.0 and not r.use_sigma
    assert r.files[:3] == ["continue-0.draw-0.mid", "continue-0.draw-1.mid", "continue-1.draw-0.mid"]
    assert G.recipe_continue([1, 0, 2], 1, target_classes=2).ca.tolist() == [2, 2, 2]
    assert G.recipe_repaint([1, 0], [0, 1]).ca.tolist() == [0, 1] and G.recipe_repaint([1, 0]).files == ["repaint-0.class-1.mid", "repaint-1.class-0.mid"]
    s, t = G.recipe_score(2, [0, 1, 2]), G.recipe_transfer(2, [0, 1, 2])
    assert s.name == "score" and s.rows == t.rows and s.a.tolist() == t.a.tolist() and s.ca.tolist() == t.ca.tolist()
    with pytest.raises(ValueError):
        G.recipe_continue([0, 1], 0)


def test_beam_search_takes_no_constraints():
    from musicstyletransfer_amd import generate as G
    from musicstyletransfer_amd.VarAutoEncoder.data import ToyData
    batch = next(iter(ToyData()))
    gen = G.LatentGenerator(None, decoder="beam")
    for call in (lambda: gen.continue_(batch, 2), lambda: gen.repaint(batch, G.hold_mask([4, 4, 4], 6)), lambda: gen.score(batch, [0]),
                 lambda: gen._decode(np.zeros((3, 8)), 6, 0, given=np.zeros((3, 6)), hold=np.zeros((3, 6)))):
        with pytest.raises(ValueError, match="beam search takes no constraints"):
            call()


def test_the_command_line_accepts_the_three_modes():
    from music_style_transfer.VarAutoEncoder import generate as G
    assert {"continue", "repaint", "score"} <= set(G.MODES)
    p = G.build_parser()
    a = p.parse_args(["--model-output", "m", "--mode", "continue", "--toy", "--prime", "3", "--n", "2", "--out", "o"])
    assert (a.mode, a.prime, a.n, a.out) == ("continue", 3, 2, "o")
    a = p.parse_args(["--model-output", "m", "--mode", "repaint", "--data", "d", "--keep-time", "4", "8", "--keep-pitch", "20", "60", "--out", "o"])
    assert (a.mode, a.keep_time, a.keep_pitch) == ("repaint", [4, 8], [20, 60])
    a = p.parse_args(["--model-output", "m", "--mode", "repaint", "--toy", "--out", "o"])
    assert a.keep_time is None and a.keep_pitch is None
    a = p.parse_args(["--model-output", "m", "--mode", "score", "--toy"])
    assert a.mode == "score" and a.out is None
    for bad in (["--model-output", "m", "--mode", "repaint", "--keep-time", "4", "--out", "o"],
                ["--model-output", "m", "--mode", "continue", "--prime", "x", "--out", "o"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for bad in (["--model-output", "m", "--mode", "continue", "--toy", "--out", "o"],   # no --prime
                ["--model-output", "m", "--mode", "repaint", "--toy"]):                 # no --out
        with pytest.raises(SystemExit):
            G.main(bad)


# ---------------------------------------------------------------------- the references
def test_frame_reference_against_a_per_cell_loop():
    rng = np.random.default_rng(5)
    N, P, tau = 3, 11, 0.7
    logits = 3.0 * rng.standard_normal((N, P))
    logits[0, 2], logits[1, 4] = 80.0, -80.0
    given = rng.integers(0, 2, (N, P)) * rng.choice([1, 255], (N, P))
    hold = rng.integers(0, 2, (N, P))
    hold[0, 2] = hold[1, 4] = 1
    given[0, 2], given[1, 4] = 0, 255  # held against a saturated logit
    free = rng.integers(0, 2, (N, P))
    frames, free_cost, held_cost = R.frame_step_held(logits, given, hold, free, tau)
    for n in range(N):
        want_free = want_held = 0.0
        for j in range(P):
            on = bool(given[n, j]) if hold[n, j] else bool(free[n, j])
            assert frames[n, j] == int(on)
            x = logits[n, j] / tau
            p = 1.0 / (1.0 + math.exp(-x)) if x > -700 else 0.0
            c = -math.log(max(p if on else 1.0 - p, 1e-30))
            if hold[n, j]:
                want_held += c
            else:
                want_free += c
        # (1 - p from its own exponential differs from 1.0 - p only in p's last digit: fp64, far below the tolerance)
        assert abs(free_cost[n] - want_free) <= 1e-9 * max(1.0, want_free) and abs(held_cost[n] - want_held) <= 1e-9 * max(1.0, want_held)
    # the floor: a held cell that contradicts a saturated logit is charged -log 1e-30, from either side
    assert R.frame_costs(80.0, tau)[1] == -math.log(1e-30) and R.frame_costs(-80.0, tau)[0] == -math.log(1e-30)
    assert held_cost[0] >= -math.log(1e-30) and held_cost[1] >= -math.log(1e-30)
    none = R.frame_step_held(logits, given, np.zeros_like(hold), free, tau)
    assert np.array_equal(none[0], free) and (none[2] == 0).all()


def test_token_reference_against_a_per_row_loop():
    rng = np.random.default_rng(6)
    N, V, eos, pad = 6, 13, 2, 0
    logits = 3.0 * rng.standard_normal((N, V))
    given = np.array([5, eos, 7, V, -1, 9])
    hold = np.array([1, 1, 0, 1, 1, 1])
    finished = np.array([False, False, False, False, False, True])
    free = np.array([3, 3, 4, 3, 3, pad])
    tok, cost, running = R.token_step_held(logits, given, hold, finished, free, eos, pad)
    assert tok.tolist() == [5, eos, 4, pad, pad, 9] and running == 3  # 5, 4 and the 9 written to a finished sequence
    for n in (0, 1):
        p = np.exp(logits[n]) / np.exp(logits[n]).sum()
        assert abs(cost[n] + math.log(p[given[n]])) < 1e-12
    assert cost[2] == 0 and cost[3] == 0 and cost[4] == 0 and cost[5] == 0  # free; out of range twice; finished
