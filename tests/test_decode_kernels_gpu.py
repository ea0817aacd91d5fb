"""The decode kernels at the lengths and beam widths decoding runs at: mst_attn_decode, mst_beam_step, mst_sample_step and
mst_beam_gather[_cols] against plain fp64 references (tests/decode_refs.py) through the C ABI, a teacher-forced DecodePlan run of
130 positions at head size 32, and beam search's device path against its host path at the script's vocabulary."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_refs as R  # noqa: E402
from decode_refs import EOS, PAD, SOS  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -7, -777.0  # what untouched int32 / fp32 memory must still hold
_DT = {torch.bfloat16: "bf16", torch.float16: "fp16"}


# ====================================================================================================== 1. mst_attn_decode
def _attn_check(gpu, B, H, dh, n_keys, dtype, mode, seed, layout=R.PACKED, kind="random"):
    """One launch against attn_decode_ref under attn_decode_tol (derived there: one ulp of the output + the fp32 sum's worst case).
    Prints the largest error as a fraction of the bound before asserting."""
    from musicstyletransfer_amd import ops as o
    D = H * dh
    cache, (ld, k_off, q_off, v_off) = R.attn_case(B, H, dh, n_keys, dtype, mode, seed, layout, kind)
    assert cache.shape[1] > n_keys and torch.isnan(cache[:, n_keys:]).all()
    ref = R.attn_decode_ref(cache, n_keys, H, dh, k_off, q_off, v_off, mode)
    tol = R.attn_decode_tol(ref, cache, n_keys, H, dh, v_off, mode)
    assert torch.isfinite(ref).all()
    # a condition on the bound, not on the kernel: the exact answer rounded to the output type lies inside it
    assert ((ref.to(dtype).double() - ref).abs() <= tol).all()
    if kind != "random":  # exp(logit) without the running maximum subtracted would be inf in fp32
        assert float(R.attn_logits(cache, n_keys, H, dh, k_off, q_off, v_off).abs().max()) > 100.0
    out = torch.full((B, D + 8), 3.0, dtype=dtype, device=gpu)  # ld_out > H dh: the pad columns keep the 3.0
    o.attn_decode(cache.to(gpu), n_keys, H, dh, k_off, q_off, v_off, out[:, :D], mode=mode)
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[:, D:] == 3.0).all(), "columns beyond H dh were written"
    got = got[:, :D].double()
    assert torch.isfinite(got).all(), "a row beyond n_keys (or a past row's Q, or a gap) reached the output"
    err = (got - ref).abs()
    print(f"attn_decode dh={dh} {_DT[dtype]} mode={mode} n={n_keys} {layout} {kind}: max err/bound = {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), (float((err / tol).max()), float(err.max()))
    return got, cache, (ld, k_off, q_off, v_off)


@pytest.mark.parametrize("n_keys", R.ATTN_NKEYS, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("mode,kind", [(0, "random"), (1, "random"), (1, "dominant")], ids=["mode0", "mode1", "mode1-logit120"])
@pytest.mark.parametrize("dtype", R.ATTN_DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("dh", R.ATTN_DH, ids=lambda d: f"dh{d}")
def test_attn_decode_matches_fp64(gpu, dh, dtype, mode, kind, n_keys):
    """B = 3, H = 2: every head size and activation type the ABI accepts, key counts on both sides of one and two waves and the longest
    decode. Rows n_keys .. t_max - 1 and the Q of past rows are NaN. Mode 1 twice: a softmax that mixes the keys (logits of order 1),
    and logits of 120 — beyond what exp takes without the running maximum — with one key holding the weight."""
    _attn_check(gpu, 3, 2, dh, n_keys, dtype, mode, seed=1000 * dh + 10 * n_keys + mode, kind=kind)


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
def test_attn_decode_at_the_decoders_size(gpu, mode):
    """bench.py --decode's launch: 256 hypotheses x 8 heads of 16, 514 cached rows"""
    _attn_check(gpu, 256, 8, 16, 514, torch.bfloat16, mode, seed=77)


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("dtype", R.ATTN_DTYPES, ids=lambda d: _DT[d])
def test_attn_decode_takes_its_offsets_from_the_arguments(gpu, dtype, mode):
    """V | gap | Q | gap | K | gap rows (ld = 3 D + 24): none of k_off, q_off, v_off, ld is the packed layout's; the gaps are NaN"""
    _attn_check(gpu, 3, 2, 32, 129, dtype, mode, seed=5, layout=R.SPREAD)
    if mode == 1:
        _attn_check(gpu, 3, 2, 32, 129, dtype, mode, seed=6, layout=R.SPREAD, kind="dominant")


@pytest.mark.parametrize("mode", [0, 1], ids=["mode0", "mode1"])
@pytest.mark.parametrize("kind", ["dominant", "uniform"])
@pytest.mark.parametrize("dtype", R.ATTN_DTYPES, ids=lambda d: _DT[d])
@pytest.mark.parametrize("dh", R.ATTN_DH, ids=lambda d: f"dh{d}")
def test_attn_decode_known_answers(gpu, dh, dtype, kind, mode):
    """logits of 120 where mode 1's answer is known without a softmax: one key dominates (the others lie at least 60 below, so p = 1
    and the output is that key's value row, exactly), or all logits are equal (the mean of the value rows). Mode 0 on the same
    caches is the plain sum."""
    n = 129
    got, cache, (ld, k_off, q_off, v_off) = _attn_check(gpu, 3, 2, dh, n, dtype, mode, seed=9, kind=kind)
    _, V, _ = R.attn_parts(cache, n, 2, dh, k_off, q_off, v_off)
    if mode == 1 and kind == "dominant":
        assert torch.equal(got, V[:, n // 2].reshape(3, -1))  # (V is already of the output type: p = 1 reproduces it exactly)
    if mode == 1 and kind == "uniform":
        mean = V.mean(1).reshape(3, -1)
        assert ((got - mean).abs() <= R.attn_decode_tol(mean, cache, n, 2, dh, v_off, 1)).all()


# ====================================================================================================== 2. mst_beam_step
def _beam_launch(gpu, probs, scores, seqs, i, K, extra=1):
    """mst_beam_step on the first B samples of buffers that hold `extra` more; probs is a column slice of a buffer LD_PAD columns
    wider whose pad columns hold 1.0. -> host copies of every output buffer, whole."""
    from musicstyletransfer_amd import ops as o
    N, V = probs.shape
    L, M = seqs.shape[1], N + extra * K
    wide = torch.full((M, V + R.LD_PAD), 1.0)
    wide[:N, :V] = torch.from_numpy(probs)
    s_in = torch.full((M,), 3.0)
    s_in[:N] = torch.from_numpy(scores)
    q_in = torch.full((M, L), 5, dtype=torch.int32)
    q_in[:N] = torch.from_numpy(seqs)
    d = {"probs": wide.to(gpu), "s_in": s_in.to(gpu), "q_in": q_in.to(gpu),
         "scores": torch.full((M,), SENT_F, device=gpu), "seqs": torch.full((M, L), SENT_I, dtype=torch.int32, device=gpu),
         "hyp_src": torch.full((M,), SENT_I, dtype=torch.int32, device=gpu), "word": torch.full((M,), SENT_I, dtype=torch.int32, device=gpu),
         "active": torch.full((L + 1,), 5, dtype=torch.int32, device=gpu)}
    o.beam_step(d["probs"][:N, :V], d["s_in"][:N], d["scores"][:N], d["q_in"][:N], d["seqs"][:N], d["hyp_src"][:N], d["word"][:N], i, K,
                EOS, PAD, active=d["active"])
    torch.cuda.synchronize()
    assert torch.equal(d["q_in"].cpu(), q_in) and torch.equal(d["s_in"].cpu().view(torch.int32), s_in.view(torch.int32)), "an input buffer was written"
    return {k: d[k].cpu().numpy() for k in ("scores", "seqs", "hyp_src", "word", "active")}


def _beam_check(got, ref, N, V, K, i, L):
    """hypotheses, words and token rows exactly; scores to rtol 1e-6 (fp32 logf, within 2 ulp, and one fp32 subtraction of
    non-negative terms: 3 x 2^-24 = 1.8e-7 of the score); active[i] exactly; everything outside the launch untouched"""
    assert ((got["hyp_src"][:N] >= 0) & (got["hyp_src"][:N] < N)).all() and ((got["word"][:N] >= 0) & (got["word"][:N] < V)).all()
    assert np.array_equal(got["hyp_src"][:N] // K, np.repeat(np.arange(N // K), K)), "a hypothesis continues another sample's"
    assert np.array_equal(got["hyp_src"][:N], ref["hyp_src"])
    assert np.array_equal(got["word"][:N], ref["word"])
    assert np.array_equal(got["seqs"][:N, :i + 1], ref["seqs"])
    fin = np.isfinite(ref["scores"])
    assert np.array_equal(np.isfinite(got["scores"][:N]), fin) and (got["scores"][:N][~fin] == np.inf).all()
    np.testing.assert_allclose(got["scores"][:N][fin], ref["scores"][fin], rtol=1e-6, atol=0)
    assert got["active"][i] == 5 + ref["alive"]
    assert (np.delete(got["active"], i) == 5).all()
    assert (got["seqs"][:N, i + 1:] == SENT_I).all(), "token columns beyond i were written"
    assert (got["seqs"][N:] == SENT_I).all() and (got["scores"][N:] == SENT_F).all()
    assert (got["hyp_src"][N:] == SENT_I).all() and (got["word"][N:] == SENT_I).all()


def _sizes(sizes):
    """parametrize arguments of (K, V) pairs, named K7-V293"""
    return {"argnames": "K,V", "argvalues": list(sizes), "ids": [f"K{k}-V{v}" for k, v in sizes]}


def _pos(name):
    return {"i1": 1, "i2": 2, "last": R.BEAM_L - 1}[name]


@pytest.mark.parametrize("pos", ["i1", "i2", "last"])
@pytest.mark.parametrize("B", [1, 64], ids=lambda b: f"B{b}")
@pytest.mark.parametrize(**_sizes(R.BEAM_SIZES))
def test_beam_step_is_the_stable_argsort(gpu, K, V, B, pos):
    """separated inputs: the reference's best 2 K scores of every sample lie at least 1e-4 (relative) apart, a thousand times what
    fp32 logf can move one — so the selection and its order must equal the fp64 reference's exactly"""
    i = _pos(pos)
    probs, scores, seqs = R.beam_separated_case(B, K, V, i, seed=100 * K + V + i)
    assert (R.beam_min_gap(probs, scores, seqs, i, K) >= R.REL_GAP).all()  # a condition on the input, for every sample
    got = _beam_launch(gpu, probs, scores, seqs, i, K)
    _beam_check(got, R.beam_step_ref(probs, scores, seqs, i, K), B * K, V, K, i, R.BEAM_L)


@pytest.mark.parametrize("setup", ["equal_scores", "first_position"])
@pytest.mark.parametrize(**_sizes(R.BEAM_SIZES))
def test_beam_step_breaks_exact_ties_by_index(gpu, K, V, setup):
    """tied candidates with bit-identical inputs (the same probability at several words, hypotheses 0 and 1 with the same row and
    score): the winners are the lowest hypothesis * V + word, in that order. first_position: hypothesis 0 at 0, the others at +inf —
    with V < K the remainder is all-infinite and must still come out as valid, distinct indices, lowest first."""
    i = 1 if setup == "first_position" else 3
    B = 5
    probs, scores, seqs = R.beam_tie_case(B, K, V, i, seed=7 * K + V, first_position=setup == "first_position")
    assert R.beam_ties_are_exact(probs, scores, seqs, i, K)
    ref = R.beam_step_ref(probs, scores, seqs, i, K)
    got = _beam_launch(gpu, probs, scores, seqs, i, K)
    _beam_check(got, ref, B * K, V, K, i, R.BEAM_L)
    cand = (got["hyp_src"][:B * K] % K) * V + got["word"][:B * K]
    for b in range(B):
        c = cand[b * K:(b + 1) * K]
        assert len(set(c.tolist())) == K, "a candidate was chosen twice"
        s = got["scores"][b * K:(b + 1) * K]
        for r in range(K - 1):  # equal scores: lowest index first
            assert s[r] < s[r + 1] or (s[r] == s[r + 1] and c[r] < c[r + 1])
    if setup == "first_position" and V < K:
        for b in range(B):
            assert np.array_equal(np.sort(cand[b * K:b * K + V]), np.arange(V))      # hypothesis 0's words, by score
            assert np.array_equal(cand[b * K + V:(b + 1) * K], np.arange(V, K))       # then the infinite ones, lowest index first
            assert np.isinf(got["scores"][b * K + V:(b + 1) * K]).all()


@pytest.mark.parametrize("i", [1, 2, 5], ids=lambda i: f"i{i}")
@pytest.mark.parametrize(**_sizes([(4, 293), (7, 293), (16, 129)]))
def test_beam_step_finished_hypotheses(gpu, K, V, i):
    """rows ending in EOS, rows ending in PAD (finished from position 2 on, live at position 1) and live rows in one sample: a
    finished hypothesis continues with PAD only, at its own score"""
    B = 6
    rng = np.random.default_rng(K + i)
    last = rng.choice(np.array([EOS, PAD, 17, 250], np.int32), size=B * K)
    last[:K] = np.resize(np.array([17, EOS, PAD, 250], np.int32), K)  # (every kind in sample 0 whatever was drawn)
    probs, scores, seqs = R.beam_separated_case(B, K, V, i, seed=31 * K + i, last=last)
    assert (R.beam_min_gap(probs, scores, seqs, i, K) >= R.REL_GAP).all()
    ref = R.beam_step_ref(probs, scores, seqs, i, K)
    got = _beam_launch(gpu, probs, scores, seqs, i, K)
    _beam_check(got, ref, B * K, V, K, i, R.BEAM_L)
    fin = (last == EOS) | ((last == PAD) & (i > 1))
    src = got["hyp_src"][:B * K]
    assert (got["word"][:B * K][fin[src]] == PAD).all()
    assert np.array_equal(got["scores"][:B * K][fin[src]], scores[src][fin[src]]), "a finished hypothesis paid for its PAD"


@pytest.mark.parametrize(**_sizes([(4, 293), (7, 293), (16, 293)]))
def test_beam_step_when_every_hypothesis_is_finished(gpu, K, V):
    """scores pass through unchanged (sorted), every word is PAD, active[i] is not touched. Second launch: one finished hypothesis with
    a finite score, the others at +inf — fewer than K finite candidates, on the general path at (16, 293): the all-infinite remainder
    comes out as the lowest remaining indices."""
    B, i = 3, 4
    last = np.resize(np.array([EOS, PAD], np.int32), B * K)
    probs, scores, seqs = R.beam_separated_case(B, K, V, i, seed=K, last=last)
    assert (R.beam_min_gap(probs, scores, seqs, i, K) >= R.REL_GAP).all()
    ref = R.beam_step_ref(probs, scores, seqs, i, K)
    got = _beam_launch(gpu, probs, scores, seqs, i, K)
    _beam_check(got, ref, B * K, V, K, i, R.BEAM_L)
    assert ref["alive"] == 0 and got["active"][i] == 5
    assert (got["word"][:B * K] == PAD).all()
    assert np.array_equal(got["scores"][:B * K], np.sort(scores.reshape(B, K), axis=1).reshape(-1))  # bit for bit
    scores = np.full((B, K), np.inf, np.float32)
    scores[:, K // 2] = 1.5
    scores = scores.reshape(-1)
    ref = R.beam_step_ref(probs, scores, seqs, i, K)
    got = _beam_launch(gpu, probs, scores, seqs, i, K)
    _beam_check(got, ref, B * K, V, K, i, R.BEAM_L)
    cand = ((got["hyp_src"][:B * K] % K) * V + got["word"][:B * K]).reshape(B, K)
    want = [(K // 2) * V + PAD] + [c for c in range(K) if c != (K // 2) * V + PAD][:K - 1]
    assert (cand == np.array(want)).all()


@pytest.mark.parametrize("nan_score_on", ["live", "finished"])
@pytest.mark.parametrize(**_sizes([(4, 293), (7, 293), (16, 128)]))
def test_beam_step_non_finite_inputs(gpu, K, V, nan_score_on):
    """a NaN probability where the best candidate was, p = 0 at the next best word (clamped at 1e-30: a finite score of 69.08 more),
    a NaN score on one hypothesis: a NaN candidate is never selected while K finite ones exist, outputs stay in range"""
    B, i = 4, 3

    def spec(rng, p, s):
        k0 = int(np.argmin(s))
        order = np.argsort(p[k0])
        p[k0, order[-1]] = np.nan
        p[k0, order[-2]] = 0.0
        s[(k0 + 1) % K] = np.nan
        return p, s

    last = np.full(B * K, 17, np.int32)
    probs, scores, seqs = R.beam_separated_case(B, K, V, i, seed=3 * K, last=last, spec=spec)
    if nan_score_on == "finished":
        nan_rows = np.where(np.isnan(scores))[0]
        seqs[nan_rows, i - 1] = EOS
    assert (R.beam_min_gap(probs, scores, seqs, i, K) >= R.REL_GAP).all()
    assert np.isnan(probs).sum() == B and np.isnan(scores).sum() == B
    ref = R.beam_step_ref(probs, scores, seqs, i, K)
    assert np.isfinite(ref["scores"]).all()  # K finite candidates exist in every sample
    got = _beam_launch(gpu, probs, scores, seqs, i, K)
    _beam_check(got, ref, B * K, V, K, i, R.BEAM_L)
    src, word = got["hyp_src"][:B * K], got["word"][:B * K]
    assert not np.isnan(probs[src, word]).any() and not np.isnan(scores[src]).any()


def test_beam_step_same_answer_on_both_sides_of_the_register_limit(gpu):
    """(8, 256) holds its 2048 scores in registers; four zero-probability columns more (8 x 260 = 2080) take the general loop. The
    zero-probability words cost 69.08 more than any other and are never chosen, so both must choose the same (hypothesis, word)
    pairs with bit-identical scores — on top of each agreeing with the reference."""
    B, K, V, i = 16, 8, 256, 9
    probs, scores, seqs = R.beam_separated_case(B, K, V, i, seed=2048)
    wide = np.concatenate([probs, np.zeros((B * K, 4), np.float32)], 1)
    res = []
    for p in (probs, wide):
        assert (R.beam_min_gap(p, scores, seqs, i, K) >= R.REL_GAP).all()
        got = _beam_launch(gpu, p, scores, seqs, i, K)
        _beam_check(got, R.beam_step_ref(p, scores, seqs, i, K), B * K, p.shape[1], K, i, R.BEAM_L)
        res.append(got)
    for k in ("hyp_src", "word", "seqs"):
        assert np.array_equal(res[0][k], res[1][k]), k
    assert np.array_equal(res[0]["scores"].view(np.uint32), res[1]["scores"].view(np.uint32))


# ====================================================================================================== 3. mst_sample_step
# A lane owns ceil(V / 64) tokens. V = 1, 5, 64: one token per lane (one, five, all lanes used); 65: two per lane, a lane with one
# token, empty lanes; 127: two, the last lane short; 293: five, a short last chunk and five empty lanes; 2051: 33, one empty lane.
SAMPLE_V = (1, 5, 64, 65, 127, 293, 2051)


@pytest.mark.parametrize("V", SAMPLE_V, ids=lambda v: f"V{v}")
def test_sample_step_follows_the_distribution(gpu, V):
    """test_device_sampling_draws_from_the_distribution's statistical form at every chunk geometry: N = 16384 sequences sharing one
    unnormalised row, counts within 6 sigma of N p (sigma of the binomial, + 1 for the rare tokens), score = -log p of the drawn
    token at rtol 1e-4 (the row sum and the division are fp32: 1e-6 of a score of order 1 to 10), a zero-probability token never"""
    from musicstyletransfer_amd import ops as o
    N, L, i = 16384, 6, 2
    g = torch.Generator().manual_seed(V)
    p = torch.rand(V, generator=g) ** 3
    zero = V // 2 if V > 1 else None
    if zero is not None:
        p[zero] = 0.0
    probs = (3.0 * p).view(1, V).repeat(N, 1).contiguous().to(gpu)
    pn = (p.double() / p.double().sum()).numpy()
    seqs = torch.full((N, L), 7, dtype=torch.int32, device=gpu)
    seqs[: N // 8, 1] = EOS
    scores = torch.zeros(N, device=gpu)
    word = torch.zeros(N, dtype=torch.int32, device=gpu)
    active = torch.zeros(L + 1, dtype=torch.int32, device=gpu)
    o.sample_step(probs, seqs, scores, word, i, 1234, EOS, PAD, active=active)
    torch.cuda.synchronize()
    tok = seqs[:, i].cpu().numpy()
    assert (tok[: N // 8] == PAD).all() and (scores[: N // 8] == 0).all()
    live = tok[N // 8:]
    assert ((live >= 0) & (live < V)).all()
    n = len(live)
    counts = np.bincount(live, minlength=V).astype(np.float64)
    assert zero is None or counts[zero] == 0
    assert (pn[live] > 0).all()
    sigma = np.sqrt(n * pn * (1 - pn)) + 1.0
    assert (np.abs(counts - n * pn) <= 6 * sigma).all(), np.abs(counts - n * pn).max()
    np.testing.assert_allclose(scores[N // 8:].cpu().numpy(), -np.log(pn[live]), rtol=1e-4, atol=1e-5)
    assert np.array_equal(word.cpu().numpy(), tok)
    assert int(active[i].item()) == int(((live != EOS) & (live != PAD)).sum())
    assert (seqs[:, :i] == 7).sum().item() == N * i - N // 8 and (seqs[:, i + 1:] == 7).all()


@pytest.mark.parametrize("V", SAMPLE_V, ids=lambda v: f"V{v}")
def test_sample_step_never_draws_a_token_without_mass(gpu, V):
    """rows whose mass sits where the chunk walk is at its edges, 1024 sequences each, in a buffer whose pad columns (ldp = V + 3)
    hold mass: all of it on the last token; on the first; inside one lane's chunk; none in the last non-empty chunk; on every other
    token. Exact: every drawn token has positive mass in its row.
    What this does NOT reach: the kernel's two rounding fallbacks (no lane owns the draw -> token V - 1; the owner's walk ends short
    -> its chunk's last token) fire only when the fp32 rounding of a lane's prefix sum straddles the target, about one draw in 1e5
    to 1e6, and the draw is a hash of (seed, position, sequence) that the ABI gives no handle on. Both take their token whatever
    its mass (docs/kernel_notes.md); the zero-mass rows here sit where they point, so a draw that did reach one would fail."""
    from musicstyletransfer_amd import ops as o
    per, L, i = 1024, 4, 1
    chunk = (V + 63) // 64
    last_lane = (V - 1) // chunk
    rng = np.random.default_rng(V)
    rows = {}
    rows["last"] = np.zeros(V)
    rows["last"][V - 1] = 2.5
    rows["first"] = np.zeros(V)
    rows["first"][0] = 0.75
    lane = last_lane // 2
    rows["one_lane"] = np.zeros(V)
    rows["one_lane"][lane * chunk:(lane + 1) * chunk] = rng.random(chunk)[: max(0, min(chunk, V - lane * chunk))] + 0.1
    if last_lane > 0:
        rows["last_chunk_empty"] = rng.random(V) + 0.05
        rows["last_chunk_empty"][last_lane * chunk:] = 0.0
    if V > 1:
        rows["every_other"] = rng.random(V) + 0.05
        rows["every_other"][1::2] = 0.0
    names = sorted(rows)
    table = np.stack([rows[k] for k in names]).astype(np.float32)
    N = per * len(names)
    wide = torch.full((N, V + 3), 50.0)
    wide[:, :V] = torch.from_numpy(np.repeat(table, per, axis=0))
    d_probs = wide.to(gpu)
    seqs = torch.full((N, L), 7, dtype=torch.int32, device=gpu)
    scores = torch.zeros(N, device=gpu)
    word = torch.full((N,), SENT_I, dtype=torch.int32, device=gpu)
    active = torch.zeros(L + 1, dtype=torch.int32, device=gpu)
    o.sample_step(d_probs[:, :V], seqs, scores, word, i, 4321, EOS, PAD, active=active)
    torch.cuda.synchronize()
    tok = seqs[:, i].cpu().numpy().reshape(len(names), per)
    sc = scores.cpu().numpy().reshape(len(names), per)
    assert ((tok >= 0) & (tok < V)).all()
    for r, name in enumerate(names):
        mass = table[r].astype(np.float64)
        assert (mass[tok[r]] > 0).all(), (name, np.unique(tok[r][mass[tok[r]] == 0]))
        np.testing.assert_allclose(sc[r], -np.log(mass[tok[r]] / mass.sum()), rtol=1e-4, atol=1e-5, err_msg=name)
    assert (tok[names.index("last")] == V - 1).all() and (tok[names.index("first")] == 0).all()
    assert (sc[names.index("last")] == 0).all()
    assert np.array_equal(word.cpu().numpy(), tok.reshape(-1))
    assert int(active[i].item()) == int(((tok != EOS) & (tok != PAD)).sum())


# ====================================================================================================== 4. mst_beam_gather[_cols]
@pytest.mark.parametrize("skip_q", [False, True], ids=["all_columns", "skip_q"])
@pytest.mark.parametrize("n_rows", [1, 513, 514], ids=lambda n: f"rows{n}")
def test_beam_gather_at_decode_size(gpu, n_rows, skip_q):
    """256 hypotheses x 514 rows of K | Q | V at D = 128 (768 bytes): from 513 rows on the grid is at its cap of 2048 workgroups and
    every thread walks the grid-stride loop. Exact: out[j, r] = in[src[j], r] for r < n_rows (without the Q third when it is skipped);
    rows from n_rows on and the skipped columns keep what they held."""
    from musicstyletransfer_amd import ops as o
    N, t_max, D = 256, 514, 128
    g = torch.Generator().manual_seed(n_rows)
    cin = torch.randint(-30000, 30000, (N, t_max, 3 * D), generator=g, dtype=torch.int16).view(torch.bfloat16).to(gpu)
    src = torch.randint(0, N, (N,), generator=g).to(torch.int32).to(gpu)
    out = torch.full_like(cin, 7.0)
    o.beam_gather(cin, out, src, n_rows, skip_cols=(D, D) if skip_q else None)
    torch.cuda.synchronize()
    want = cin[src.long(), :n_rows].view(torch.int16)  # (bit patterns: a NaN pattern must compare equal to itself)
    got = out.view(torch.int16)
    sent = torch.full((1,), 7.0, dtype=torch.bfloat16).view(torch.int16).item()
    assert (got[:, n_rows:] == sent).all()
    if skip_q:
        assert torch.equal(got[:, :n_rows, :D], want[:, :, :D]) and torch.equal(got[:, :n_rows, 2 * D:], want[:, :, 2 * D:])
        assert (got[:, :, D:2 * D] == sent).all()
    else:
        assert torch.equal(got[:, :n_rows], want)


# ====================================================================================================== 5. a long teacher-forced decode
@pytest.mark.parametrize("attention", ["query", "key"])
@pytest.mark.parametrize("kind", ["token", "pianoroll"])
def test_long_decode_matches_the_oracle(gpu, kind, attention):
    """test_decode_step_matches_the_oracle's method at 130 positions, decoder width 128 x 4 heads (dh = 32), B = 4: the same tokens /
    frames through DecodePlan and through oracle.decode_incremental (fp32, on the values the kernels read). Bound: mean and max |dp|
    at most TWICE decode_refs.STORAGE_COST — the error the fp32 oracle itself shows when its weights are rounded to bf16:
        token / query 8.54e-5, 1.66e-3   token / key 1.17e-4, 4.41e-3   pianoroll / query 6.98e-4, 3.80e-3   pianoroll / key 1.15e-3, 1.79e-2
    Then a second pass over the same plan replays the captured graphs and is bit-identical."""
    from musicstyletransfer_amd import decode, engine as E
    O, ocfg, params, z, classes, fed = R.long_decode_inputs(kind)
    dims, B, n = R.LONG_DIMS[kind], R.LONG_B, R.LONG_N
    Dd = dims[7]
    store = E.ParamStore(E.VAEConfig(kind, *dims), gpu, torch.bfloat16, params_np=params)
    want = R.long_decode_oracle(O, ocfg, store.as_consumed_numpy(), z, classes, fed, attention)
    pos = O.positional_encodings(Dd, 1)[0].astype(np.float32)
    init = z @ params["decoder.latent2hid.weight"].T + params["decoder.latent2hid.bias"] + params["decoder.class2hid.weight"][classes]
    row0 = torch.from_numpy((np.sqrt(Dd) * init + pos).astype(np.float32)).to(torch.bfloat16).to(gpu)
    plan = decode.DecodePlan(store, B, n + 1, attention=attention)
    assert plan.cfg.d_model // plan.cfg.d_heads == 32
    plan.start(row0)
    got = np.stack([plan.step(fed[:, t]).float().cpu().numpy() for t in range(n)], 1)
    err = np.abs(got - want)
    cost = R.STORAGE_COST[(kind, attention)]
    print(f"long decode {kind} / {attention}: mean |dp| {err.mean():.3e} (bound {2 * cost[0]:.3e}), max {err.max():.3e} (bound {2 * cost[1]:.3e})")
    assert err.mean() <= 2 * cost[0] and err.max() <= 2 * cost[1], (err.mean(), err.max())
    if kind == "token":
        np.testing.assert_allclose(got.sum(-1), 1.0, atol=1e-3)
    assert plan.t == n
    assert plan.use_graphs and sorted(plan._graphs) == list(range(2, n + 1))
    plan.reset()
    plan.start(row0)
    again = np.stack([plan.step(fed[:, t]).float().cpu().numpy() for t in range(n)], 1)
    assert sorted(plan._graphs) == list(range(0, n + 1))
    assert np.array_equal(again, got)


# ====================================================================================================== 6. beam search: device path vs host path
@pytest.fixture(scope="module")
def script_vocabulary_model(gpu):
    """an untrained token model at the script's vocabulary (V = 293), decoder 128 x 4 heads, and a batch of 3 sequences of 36 tokens:
    beam search runs to 72 positions, past one wave of cached rows"""
    from musicstyletransfer_amd.MIDIUtil.defaults import NUM_EVENTS
    from musicstyletransfer_amd.VarAutoEncoder import model as M
    from musicstyletransfer_amd.VarAutoEncoder.data import Batch
    from musicstyletransfer_amd.VarAutoEncoder.transformer import TransformerConfig
    from musicstyletransfer_amd.VarAutoEncoder.utils import gpu as gpu_ctx
    assert NUM_EVENTS == 293
    cfg = M.ModelConfig(M.EncoderConfig(TransformerConfig(64, 0.2, 1, 4, NUM_EVENTS), 16, 2, NUM_EVENTS),
                        M.DecoderConfig(TransformerConfig(128, 0.2, 1, 4, NUM_EVENTS), 16, 2, NUM_EVENTS))
    m = M.Model(cfg).initialize(gpu_ctx(0), seed=1234)
    rng = np.random.default_rng(1234)
    B, T1 = 3, 36
    tokens = rng.integers(3, NUM_EVENTS, size=(B, T1))
    tokens[:, 0] = SOS
    return m, Batch([tokens, np.full(B, T1), rng.integers(0, 2, size=B)], [np.zeros_like(tokens)])


@pytest.mark.parametrize("K", [4, 8, 16], ids=lambda k: f"beam{k}")
def test_beam_search_on_the_device_equals_the_host_loop(gpu, script_vocabulary_model, K):
    """test_samplers_on_the_toy_model's comparison (equal hypotheses; scores to rtol 2e-4 as there) where the device path differs from
    the toy's: V = 293, beams on both paths of mst_beam_step (4 x 293 in registers; 8 and 16 x 293 in the general loop), at least 70
    positions"""
    from musicstyletransfer_amd.VarAutoEncoder import sampler as S
    m, batch = script_vocabulary_model
    dev_s, host_s = S.BeamSearchSampler(beam_size=K, on_device=True), S.BeamSearchSampler(beam_size=K, on_device=False)
    for smp in (dev_s, host_s):
        smp.update_parameters(m)
        smp.sample(batch)
    assert dev_s.hypotheses.shape == host_s.hypotheses.shape == (3, K, 72)
    assert min(dev_s.positions_decoded, host_s.positions_decoded) >= 70
    np.testing.assert_allclose(dev_s.scores, host_s.scores, rtol=2e-4, atol=2e-4)
    assert np.array_equal(dev_s.hypotheses, host_s.hypotheses), K
    assert (np.diff(dev_s.scores, axis=1) >= 0).all()
