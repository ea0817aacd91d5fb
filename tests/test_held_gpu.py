"""Constrained decoding on the GPU: mst_frame_step_held and mst_token_step_held against the unconstrained launches (bitwise where
nothing is held, and in every free cell) and against the fp64 references of tests/held_refs.py; the constrained FrameSampling loop
against a host loop and against the oracle; continue_ / repaint / score and the command line on the toy token model.

Tolerances are the project's for these sums: rtol 1e-4, atol 1e-5 for a score against fp64 (test_frame_step_draws_from_the_
distribution, test_token_step_gpu.py); mean <= 3e-3, max <= 6e-2 for probabilities against the oracle
(test_transfer_matches_the_oracle)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import held_refs as R  # noqa: E402
from test_generate_gpu import _pianoroll_model  # noqa: E402

pytestmark = pytest.mark.gpu

EOS, PAD, SOS = 2, 0, 1
DTYPES = [torch.bfloat16, torch.float16]
_DT = {torch.bfloat16: "bf16", torch.float16: "fp16"}
FLOOR_COST = -np.log(1e-30)


# ====================================================================================================== 1. mst_frame_step_held
class FrameBench:
    """N sequences of P logits (3 randn, column 3 at +80 and column 5 at -80) in rows of ld; the pad columns of logits, given and hold
    hold junk that would show if it were read. L = 5."""
    L = 5

    def __init__(self, gpu, adt, N, P, ld):
        self.gpu, self.adt, self.N, self.P, self.ld = gpu, adt, N, P, ld
        g = torch.Generator().manual_seed(N * 1000 + P)
        logits = (3.0 * torch.randn(N, ld, generator=g)).to(adt)
        logits[:, 3], logits[:, 5] = 80.0, -80.0
        logits[:, P:] = 50.0
        self.logits = logits.to(gpu)
        self.x64 = logits[:, :P].double().numpy()  # the stored values
        given = torch.randint(0, 2, (N, self.L, ld), generator=g) * (1 + 254 * torch.randint(0, 2, (N, self.L, ld), generator=g))
        assert (given == 255).any() and (given == 1).any() and (given == 0).any()
        given[:, :, 3], given[:, :, 5] = 0, 255  # against the saturated logits
        given[:, :, P:] = 255
        self.given = given.to(torch.uint8)
        self.seed = torch.tensor([4321], dtype=torch.int64, device=gpu)

    def hold(self, kind):
        N, L, ld, P = self.N, self.L, self.ld, self.P
        if kind == "none":
            h = torch.zeros(N, L, ld, dtype=torch.uint8)
        elif kind == "all":
            h = torch.full((N, L, ld), 255, dtype=torch.uint8)
            h[:, :, 1:P:2] = 1  # any non-zero byte holds
        else:
            h = torch.randint(0, 2, (N, L, ld), generator=torch.Generator().manual_seed(7)).to(torch.uint8) * 3
        if kind == "none":
            h[:, :, P:] = 1  # junk behind the row: must not hold anything, must not be read
        return h

    def launch(self, i, hold=None, tau=1.0, mode="draw", thr=0.5):
        """hold None: mst_frame_step. Every output starts from a pattern, so a stray write shows."""
        from musicstyletransfer_amd import ops as o
        N, L, ld, P, gpu = self.N, self.L, self.ld, self.P, self.gpu
        frames = torch.full((N, ld), 9, dtype=torch.uint8, device=gpu)
        roll = torch.full((N, L, ld), 7, dtype=torch.uint8, device=gpu)
        scores = torch.full((N,), 0.5, device=gpu)
        held = torch.full((N,), 0.25, device=gpu)
        probs = torch.full((N, L, P), -1.0, device=gpu)
        if hold is None:
            o.frame_step(self.logits, P, i, self.seed, frames, roll, scores, tau=tau, mode=mode, thr=thr, probs_out=probs)
        else:
            o.frame_step_held(self.logits, P, i, self.seed, frames, roll, scores, self.given.to(gpu), hold.to(gpu), held, tau=tau,
                              mode=mode, thr=thr, probs_out=probs)
        torch.cuda.synchronize()
        out = dict(frames=frames.cpu(), roll=roll.cpu(), scores=scores.cpu(), held=held.cpu(), probs=probs.cpu())
        # rows of the roll other than i - 1, columns >= P of the frames and of the roll's row, other rows of probs: untouched
        other = [k for k in range(L) if k != i - 1]
        assert (out["roll"][:, other] == 7).all() and (out["probs"][:, other] == -1.0).all()
        assert (out["frames"][:, P:] == 9).all() and (out["roll"][:, i - 1, P:] == 7).all()
        assert torch.equal(out["frames"][:, :P], out["roll"][:, i - 1, :P]) and (out["frames"][:, :P] <= 1).all()
        return out


FRAME_CASES = [(adt, N, P, ld) for adt in DTYPES for N in (1, 6) for P, ld in ((45, 48), (130, 136))]


@pytest.mark.parametrize("adt,N,P,ld", FRAME_CASES, ids=[f"{_DT[a]}-N{n}-P{p}" for a, n, p, _ in FRAME_CASES])
def test_frame_step_held(gpu, adt, N, P, ld):
    b = FrameBench(gpu, adt, N, P, ld)
    for i in (1, 3, 4):
        for tau, mode in ((1.0, "draw"), (0.7, "threshold")):
            case = (i, tau, mode)
            free = b.launch(i, None, tau, mode)
            # ---- nothing held: mst_frame_step bit for bit, held_scores as they were
            got = b.launch(i, b.hold("none"), tau, mode)
            for k in ("frames", "roll", "scores", "probs"):
                assert torch.equal(got[k], free[k]), (case, k)
            assert (got["held"] == 0.25).all(), case
            assert (free["scores"] != 0.5).all()
            given = b.given[:, i - 1, :P].numpy()
            f_free = free["frames"][:, :P].numpy()
            # ---- everything held
            got = b.launch(i, b.hold("all"), tau, mode)
            assert np.array_equal(got["frames"][:, :P].numpy(), (given != 0).astype(np.uint8)), case
            assert (got["scores"] == 0.5).all(), case  # no free cell: nothing added
            assert torch.equal(got["probs"], free["probs"]), case
            frames, c_free, c_held = R.frame_step_held(b.x64, given, np.ones_like(given), f_free, tau)
            on, off = R.frame_costs(b.x64, tau)
            assert (off[:, 3] == FLOOR_COST).all() and (on[:, 5] == FLOOR_COST).all()  # the two contradicted cells: -log 1e-30 each
            assert (c_free == 0).all() and (c_held >= 2 * FLOOR_COST).all()
            np.testing.assert_allclose(got["held"].double().numpy() - 0.25, c_held, rtol=1e-4, atol=1e-5, err_msg=str(case))
            # ---- a random half
            hold = b.hold("half")
            h = hold[:, i - 1, :P].numpy() != 0
            assert h.any() and (~h).any()
            got = b.launch(i, hold, tau, mode)
            g = got["frames"][:, :P].numpy()
            assert np.array_equal(g[h], (given != 0)[h].astype(np.uint8)), case
            assert np.array_equal(g[~h], f_free[~h]), case  # a free cell's draw does not depend on which others are held
            assert torch.equal(got["probs"], free["probs"]), case
            frames, c_free, c_held = R.frame_step_held(b.x64, given, h, f_free, tau)
            assert np.array_equal(g, frames)
            np.testing.assert_allclose(got["scores"].double().numpy() - 0.5, c_free, rtol=1e-4, atol=1e-5, err_msg=str(case))
            np.testing.assert_allclose(got["held"].double().numpy() - 0.25, c_held, rtol=1e-4, atol=1e-5, err_msg=str(case))


# ====================================================================================================== 2. mst_token_step_held
class TokenBench:
    """N = 5 sequences with their own logit rows in a buffer of ldl = roundup8(V) + 8 whose pad columns hold the dtype's largest finite
    value; sequence 1 has ended before the position. L = 6."""
    N, L = 5, 6

    def __init__(self, gpu, adt, V):
        self.gpu, self.V = gpu, V
        g = torch.Generator().manual_seed(V)
        ldl = (V + 7) // 8 * 8 + 8
        logits = torch.full((self.N, ldl), torch.finfo(adt).max, dtype=adt)
        logits[:, :V] = (3.0 * torch.randn(self.N, V, generator=g)).to(adt)
        self.logits = logits.to(gpu)
        self.x64 = logits[:, :V].double().numpy()
        self.seed = torch.tensor([99], dtype=torch.int64, device=gpu)
        self.finished = np.array([False, True, False, False, False])

    def launch(self, i, given=None, hold=None, tau=1.0, top_k=0, top_p=1.0, seqs=None):
        """hold None: mst_token_step. given: [N] tokens of position i; hold: [N] flags."""
        from musicstyletransfer_amd import ops as o
        N, L, gpu = self.N, self.L, self.gpu
        if seqs is None:
            seqs = torch.full((N, L), 7, dtype=torch.int32)
            seqs[1, i - 1] = EOS
        seqs = seqs.clone().to(gpu)
        before = seqs.cpu().numpy().copy()
        scores = torch.full((N,), 0.5, device=gpu)
        held = torch.full((N,), 0.25, device=gpu)
        word = torch.full((N,), -7, dtype=torch.int32, device=gpu)
        active = torch.zeros(L + 1, dtype=torch.int32, device=gpu)
        kept = torch.full((N,), -7, dtype=torch.int32, device=gpu)
        kw = dict(tau=tau, top_k=top_k, top_p=top_p, active=active, kept_out=kept)
        if hold is None:
            o.token_step(self.logits, self.V, i, self.seed, seqs, scores, word, EOS, PAD, **kw)
        else:
            gv = torch.full((N, L), -12345, dtype=torch.int32)  # (other positions' entries: never read)
            hd = torch.full((N, L), 1, dtype=torch.uint8)
            gv[:, i] = torch.as_tensor(np.asarray(given), dtype=torch.int32)
            hd[:, i] = torch.as_tensor(np.asarray(hold), dtype=torch.uint8)
            o.token_step_held(self.logits, self.V, i, self.seed, seqs, scores, word, EOS, PAD, gv.to(gpu), hd.to(gpu), held, **kw)
        torch.cuda.synchronize()
        out = dict(seqs=seqs.cpu().numpy(), scores=scores.cpu().numpy(), held=held.cpu().numpy(), word=word.cpu().numpy(),
                   active=active.cpu().numpy(), kept=kept.cpu().numpy())
        cols = [k for k in range(L) if k != i]
        assert np.array_equal(out["seqs"][:, cols], before[:, cols])  # only column i is written
        assert np.array_equal(out["seqs"][:, i], out["word"])
        assert (out["active"][[k for k in range(L + 1) if k != i]] == 0).all()
        return out


TOKEN_CASES = [(adt, V) for adt in DTYPES for V in (45, 130, 520)]  # 520: the form that walks memory


@pytest.mark.parametrize("adt,V", TOKEN_CASES, ids=[f"{_DT[a]}-V{v}" for a, v in TOKEN_CASES])
def test_token_step_held(gpu, adt, V):
    b = TokenBench(gpu, adt, V)
    N = b.N
    for i in (1, 2, 4):
        # ---- nothing held: mst_token_step bit for bit
        for tau, top_k, top_p in ((1.0, 0, 1.0), (0.7, 5, 0.9)):
            free = b.launch(i, tau=tau, top_k=top_k, top_p=top_p)
            got = b.launch(i, given=[V + 5] * N, hold=[0] * N, tau=tau, top_k=top_k, top_p=top_p)
            for k in ("seqs", "scores", "word", "active", "kept"):
                assert np.array_equal(got[k], free[k]), (i, tau, k)
            assert (got["held"] == 0.25).all()
            assert free["seqs"][1, i] == PAD and (free["kept"] > 0).all()
        # ---- everything held (sequence 1 has ended: written all the same, charged nothing; sequence 3 is given its EOS)
        given = np.array([V - 1, 9, 5, EOS, 11])
        got = b.launch(i, given=given, hold=[1, 255, 1, 3, 1], tau=0.7, top_k=5, top_p=0.9)
        assert np.array_equal(got["seqs"][:, i], given) and np.array_equal(got["word"], given)
        assert (got["scores"] == 0.5).all() and (got["kept"] == 0).all()
        assert got["active"][i] == 4  # every token but the EOS, the one written to the finished sequence included
        tok, cost, running = R.token_step_held(b.x64, given, [1] * N, b.finished, free["seqs"][:, i], EOS, PAD)
        assert np.array_equal(tok, given) and running == 4 and cost[1] == 0 and (cost[[0, 2, 3, 4]] > 0).all()
        np.testing.assert_allclose(got["held"].astype(np.float64) - 0.25, cost, rtol=1e-4, atol=1e-5)
        assert got["held"][1] == 0.25
        # ---- some held: the others are the unconstrained launch's
        hold = np.array([1, 0, 0, 1, 0])
        got = b.launch(i, given=given, hold=hold)
        free = b.launch(i)
        tok, cost, running = R.token_step_held(b.x64, given, hold, b.finished, free["seqs"][:, i], EOS, PAD)
        assert np.array_equal(got["seqs"][:, i], tok) and got["active"][i] == running
        assert np.array_equal(got["scores"][hold == 0], free["scores"][hold == 0]) and (got["scores"][hold == 1] == 0.5).all()
        assert np.array_equal(got["kept"], np.where(hold == 1, 0, free["kept"]))
        np.testing.assert_allclose(got["held"].astype(np.float64) - 0.25, cost, rtol=1e-4, atol=1e-5)


def test_a_free_position_behind_a_held_eos_writes_pad(gpu):
    b = TokenBench(gpu, torch.bfloat16, 45)
    first = b.launch(2, given=[EOS, 5, EOS, 6, 7], hold=[1] * 5)
    after = b.launch(3, given=[9] * 5, hold=[0] * 5, seqs=torch.from_numpy(first["seqs"]))
    assert after["seqs"][[0, 2], 3].tolist() == [PAD, PAD] and (after["scores"][[0, 2]] == 0.5).all()
    # the others drew and were charged — sequence 1 too: it was given a token behind its end, so position 3 sees it running
    assert (after["scores"][[1, 3, 4]] > 0.5).all() and after["active"][3] == ((after["seqs"][:, 3] != EOS) & (after["seqs"][:, 3] != PAD)).sum()


def test_an_out_of_range_given_token_writes_pad_and_charges_nothing(gpu):
    """never an index outside the row: the kernel writes PAD; scores and held_scores stay as they were (run once)"""
    b = TokenBench(gpu, torch.bfloat16, 45)
    got = b.launch(2, given=[45, -1, 1 << 30, -(1 << 31), 45 + 8], hold=[1] * 5)
    assert (got["seqs"][:, 2] == PAD).all() and (got["word"] == PAD).all()
    assert (got["scores"] == 0.5).all() and (got["held"] == 0.25).all() and (got["kept"] == 0).all() and got["active"][2] == 0


# ====================================================================================================== 3. the constrained loop
B, L, P, DD = 5, 12, 48, 32


def _row0(m, rng, gpu):
    return torch.from_numpy(rng.standard_normal((B, DD)).astype(np.float32)).to(m.store.act_dtype).to(gpu)


def test_an_empty_mask_is_the_unconstrained_run(gpu):
    from musicstyletransfer_amd import decode
    _, _, _, m, rng = _pianoroll_model(gpu)
    row0 = _row0(m, rng, gpu)
    fs = decode.FrameSampling(m.store, B, L, attention="query")
    r0, s0 = fs.run(row0, mode="draw", seed=5)
    keys = set(fs._graphs)
    given = rng.integers(0, 2, (B, L - 1, P)).astype(np.uint8)
    r1, s1 = fs.run(row0, mode="draw", seed=5, given=given, hold=np.zeros_like(given))
    assert np.array_equal(r0, r1) and np.array_equal(s0, s1) and 0 < r0.mean() < 1
    assert fs.held_scores.shape == (B,) and (fs.held_scores == 0).all()
    assert keys < set(fs._graphs) and len(fs._graphs) == 2 * len(keys)  # the unconstrained keys are as they were
    r2, s2 = fs.run(row0, mode="draw", seed=5)
    assert np.array_equal(r0, r2) and np.array_equal(s0, s2) and len(fs._graphs) == 2 * len(keys)
    with pytest.raises(ValueError):
        fs.run(row0, given=given)
    with pytest.raises(ValueError):
        fs.run(row0, given=given[:, :, :40], hold=given[:, :, :40])


@pytest.mark.parametrize("attention,causal", [("query", False), ("key", False), ("key", True)])
def test_a_continuation_is_the_host_loop_fed_the_opening(gpu, attention, causal):
    """threshold mode; the opening is the COMPLEMENT of what the unconstrained run writes there, so every held cell differs from what
    the model would have written and the test cannot pass without the constraint. Exact, as test_frame_sampling_loop_is_the_host_loop."""
    from musicstyletransfer_amd import decode
    _, _, _, m, rng = _pianoroll_model(gpu, causal=causal)
    st = m.store
    row0 = _row0(m, rng, gpu)
    fs = decode.FrameSampling(st, B, L, attention=attention)
    free, _ = fs.run(row0, mode="threshold", thr=0.5)
    prime = 5
    given = np.zeros((B, L - 1, P), np.uint8)
    given[:, :prime] = 1 - free[:, :prime]
    hold = np.zeros_like(given)
    hold[:, :prime] = 1
    got, scores = fs.run(row0, mode="threshold", thr=0.5, given=given, hold=hold)
    assert got.shape == (B, L - 1, P) and np.array_equal(got[:, :prime], given[:, :prime])
    plan = decode.DecodePlan(st, B, L, attention=attention)
    plan.start(row0)
    prev = np.zeros((B, P), np.uint8)
    prev[:, 0] = 1
    want = []
    for i in range(1, L):
        plan.step(prev)
        torch.cuda.synchronize()
        prev = given[:, i - 1] if i - 1 < prime else (plan.logits[:, :P].float() > 0).to(torch.uint8).cpu().numpy()
        want.append(prev)
    want = np.stack(want, 1)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[:, prime:], free[:, prime:])  # the opening reached the continuation
    assert np.isfinite(scores).all() and np.isfinite(fs.held_scores).all() and (fs.held_scores > 0).all()


def test_a_held_pitch_band(gpu):
    from musicstyletransfer_amd import decode
    _, _, _, m, rng = _pianoroll_model(gpu)
    row0 = _row0(m, rng, gpu)
    fs = decode.FrameSampling(m.store, B, L, attention="query")
    given = rng.integers(0, 2, (B, L - 1, P)).astype(np.uint8)
    hold = np.zeros_like(given)
    hold[:, :, 24:] = 1
    a, sa = fs.run(row0, mode="draw", seed=1, given=given, hold=hold)
    n_graphs = len(fs._graphs)
    assert n_graphs == L - 1
    b, sb = fs.run(row0, mode="draw", seed=2, given=given, hold=hold)
    c, sc = fs.run(row0, mode="draw", seed=1, given=given, hold=hold)
    held_c = fs.held_scores.copy()
    for r in (a, b, c):
        assert np.array_equal(r[:, :, 24:], given[:, :, 24:])
    assert not np.array_equal(a[:, :, :24], b[:, :, :24])
    assert np.array_equal(a, c) and np.array_equal(sa, sc)
    # another mask and another piece: device data, nothing new is captured
    given2 = 1 - given
    hold2 = np.zeros_like(given)
    hold2[:, 3:7, :30] = 1
    d, _ = fs.run(row0, mode="draw", seed=1, given=given2, hold=hold2)
    assert len(fs._graphs) == n_graphs
    assert np.array_equal(d[:, 3:7, :30], given2[:, 3:7, :30]) and not np.array_equal(d[:, :, 24:], given[:, :, 24:])
    assert not np.array_equal(fs.held_scores, held_c)


@pytest.mark.parametrize("attention", ["query", "key"])
def test_score_matches_the_oracle(gpu, attention):
    """score() over both classes on the sizes of test_transfer_matches_the_oracle (B 5, 9 positions): B * 2 rows in transfer's order;
    the per-position probabilities match oracle.decode_incremental fed the same frames within that test's bound; held_scores is the
    fp64 sum over the held cells formed from the device's own kept probabilities."""
    from musicstyletransfer_amd import generate as G
    from music_style_transfer.VarAutoEncoder.data import Batch
    O, ocfg, params, m, rng = _pianoroll_model(gpu)
    n = 9
    batch = O.synthetic_pianoroll_batch(rng, B, n, P, num_classes=2, density=0.1, ragged=True)
    x, lens, cls, labels = (batch[k].numpy() for k in ("x", "seq_lens", "classes", "labels"))
    one = Batch([x, lens, cls], [labels])
    gen = G.LatentGenerator(m, attention=attention, decoder="greedy", keep_probs=True)
    mu, _ = gen.encode(one)
    res = gen.score(one, [0, 1])
    ref = gen.transfer(one, [0, 1], length=n + 1)
    assert len(res) == 2 * B and res.rows == ref.rows and res.name == "score"
    assert [(r["melody"], r["cls"]) for r in res.rows] == [(b, c) for b in range(B) for c in (0, 1)]
    mel = np.array([r["melody"] for r in res.rows])
    target = np.array([r["cls"] for r in res.rows])
    assert np.array_equal(res.z, mu.cpu().numpy()[mel])
    want_hold = G.hold_mask(lens, n, P)[mel]
    assert res.rolls.shape == (2 * B, n, P) and res.probs.shape == (2 * B, n, P) and np.array_equal(res.hold, want_hold)
    assert np.array_equal(res.rolls[want_hold], labels[mel][want_hold])  # the piece itself, up to every row's length
    assert np.array_equal(res.rolls[~want_hold], (res.probs > 0.5).astype(np.uint8)[~want_hold])  # behind it: greedy
    start = np.zeros((2 * B, 1, P), np.uint8)
    start[:, 0, 0] = 1
    fed = np.concatenate([start, res.rolls[:, : n - 1]], 1)
    Pm = O.to_torch_params(m.store.as_consumed_numpy(), requires_grad=False)
    want = O.decode_incremental(Pm, ocfg, torch.from_numpy(res.z), torch.from_numpy(target), torch.from_numpy(fed), attention).numpy()
    err = np.abs(res.probs - want)
    print("score vs oracle: mean", err.mean(), "max", err.max())
    assert err.mean() <= 3e-3 and err.max() <= 6e-2, (err.mean(), err.max())
    p = res.probs.astype(np.float64)
    cost = -np.log(np.maximum(np.where(res.rolls > 0, p, 1.0 - p), 1e-30))
    held = np.where(want_hold, cost, 0.0).sum((1, 2))
    free = np.where(want_hold, 0.0, cost).sum((1, 2))
    print("held scores:", res.held_scores, "fp64 from the kept probabilities:", held)
    np.testing.assert_allclose(res.held_scores, held, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(res.scores, free, rtol=1e-4, atol=1e-5)
    assert (res.held_scores > 0).all()
    # chunked: the same rows, two at a time
    gen2 = G.LatentGenerator(m, attention=attention, decoder="greedy", keep_probs=True, max_rows=4)
    res2 = gen2.score(one, [0, 1])
    assert np.array_equal(res2.rolls[want_hold], res.rolls[want_hold]) and np.array_equal(res2.hold, res.hold)
    np.testing.assert_allclose(res2.held_scores, res.held_scores, rtol=1e-4, atol=1e-5)


# ====================================================================================================== 4. the token ends, the command line
@pytest.fixture(scope="module")
def toy(gpu, tmp_path_factory):
    """the toy token model, trained as test_interface_on_the_toy_model trains it (fewer steps: nothing below needs a good model)"""
    from music_style_transfer.VarAutoEncoder import main, utils
    root = tmp_path_factory.mktemp("held_toy")
    t = main.main(["--toy", "--gpu", "--max-steps", "60", "--model-output", str(root)])
    t.stream.synchronize()
    torch.cuda.synchronize()
    folder = os.path.join(str(root), "model")
    utils.save_model(t.model, os.path.join(folder, "params.0"))
    return t, folder, root


def test_continue_repaint_and_score_on_the_toy_model(toy):
    from music_style_transfer.VarAutoEncoder import generate as G
    from music_style_transfer.VarAutoEncoder.data import ToyData
    t, _, _ = toy
    data = ToyData()
    batch = next(iter(data))
    for decoder in ("sampling", "greedy"):
        gen = G.LatentGenerator(t.model, seed=3, decoder=decoder)
        out = gen.continue_(batch, prime=3)
        assert out.sequences.shape == (3, 10) and np.array_equal(out.sequences[:, :3], data.tokens[:, :3])
        assert np.array_equal(out.sequences[:, 1:4], data.labels[:, :3])  # SOS, then the three held tokens
        assert np.isfinite(out.scores).all() and np.isfinite(out.held_scores).all() and (out.held_scores > 0).all()
        assert out.hold.shape == (3, 6) and out.hold[:, 1:4].all() and not out.hold[:, 0].any() and not out.hold[:, 4:].any()
        assert ((out.sequences >= 0) & (out.sequences < 10)).all()
        two = gen.continue_(batch, prime=3, n_per_sample=2)
        assert len(two) == 6 and [r["melody"] for r in two.rows] == [0, 0, 1, 1, 2, 2]
        assert np.array_equal(two.sequences[:, 1:4], np.repeat(data.labels[:, :3], 2, 0))
        assert np.array_equal(two.held_scores[0::2], two.held_scores[1::2]) and np.isfinite(two.scores).all()
        # an opening longer than the melody stops short of its EOS (seq_len 4: SOS and three tokens)
        long = gen.continue_(batch, prime=9, length=8)
        assert long.hold[:, 1:4].all() and not long.hold[:, 4:].any()
        sc = gen.score(batch)
        assert len(sc) == 9 and sc.held_scores.shape == (9,) and np.isfinite(sc.held_scores).all() and (sc.held_scores > 0).all()
        assert np.array_equal(sc.sequences[:, :5], np.repeat(G.token_piece(data.tokens, data.seq_lens)[:, :5], 3, 0))
        rp = gen.repaint(batch, G.hold_mask(data.seq_lens + 1, 6, time=(2, 4)), target_classes=1)
        assert np.array_equal(rp.sequences[:, 2:4], data.labels[:, 1:3]) and [r["cls"] for r in rp.rows] == [1, 1, 1]
    ts = t.model.token_sampling_plan(3, 6)
    with pytest.raises(ValueError):
        ts.run(torch.zeros(3, 32, dtype=t.model.store.act_dtype, device=t.model.store.device), given=np.full((3, 6), 10), hold=np.ones((3, 6)))
    with pytest.raises(ValueError, match="beam search takes no constraints"):
        G.LatentGenerator(t.model, decoder="beam").continue_(batch, prime=2)


def test_the_command_line(toy, capsys):
    from music_style_transfer.VarAutoEncoder import generate as G
    from music_style_transfer.MIDIUtil import smf
    _, folder, root = toy
    common = ["--model-output", folder, "--checkpoint", "-1", "--toy", "--length", "10", "--seed", "1"]
    for mode, extra, n_files in (("continue", ["--prime", "2", "--n", "2"], 6), ("repaint", ["--keep-time", "1", "3"], 3)):
        out = str(root / ("cli-" + mode))
        files = G.main(common + ["--mode", mode, "--out", out] + extra)
        assert len(files) == n_files and sorted(os.listdir(out)) == sorted(os.path.basename(f) for f in files)
        for f in files:
            assert os.path.getsize(f) > 0 and len(list(smf.read_midifile(f))) == 1  # one track, parseable
    capsys.readouterr()
    before = set(os.listdir(str(root)))
    lines = G.main(["--model-output", folder, "--toy", "--mode", "score"])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("melody ")]
    assert len(lines) == 9 and printed == lines and set(os.listdir(str(root))) == before  # B * C lines, no files
    assert lines[0].startswith("melody 0 class 0 nll ") and lines[8].startswith("melody 2 class 2 nll ")
    assert all(np.isfinite(float(ln.split()[-1])) for ln in lines)
