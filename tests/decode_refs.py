"""Plain fp64 references and input generators for the decode kernels (mst_attn_decode, mst_beam_step). CPU only: imported by
tests/test_decode_kernels_gpu.py, which compares the kernels with them, and by tests/test_decode_refs_cpu.py, which keeps the
references and the generators honest on a machine without a GPU. Nothing here launches the library."""
import numpy as np
import torch

EOS, PAD, SOS = 2, 0, 1  # MIDIUtil.defaults (asserted in test_decode_refs_cpu.py)
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# ------------------------------------------------------------------------------------------------ mst_attn_decode
ATTN_DH = (16, 32, 64)
ATTN_DTYPES = (torch.bfloat16, torch.float16)
ATTN_NKEYS = (1, 2, 63, 64, 65, 128, 129, 514)  # around one wave (64 lanes), around two, and the longest decode (2 (T + 1) = 514)
PACKED = "packed"   # K | Q | V at (0, D, 2 D), rows of 3 D: the layout DecodePlan uses
SPREAD = "spread"   # V | gap | Q | gap | K | gap: every offset differs from the packed layout's


def attn_layout(D, layout):
    """-> (ld, k_off, q_off, v_off)"""
    return (3 * D, 0, D, 2 * D) if layout == PACKED else (3 * D + 24, 2 * D + 16, D + 8, 0)


def attn_case(B, H, dh, n_keys, dtype, mode, seed, layout=PACKED, kind="random", t_pad=3):
    """A cache [B, t_max, ld] of `dtype` whose only finite entries are the ones the kernel may read: K and V of rows < n_keys and Q of
    row n_keys - 1. Everything else — rows n_keys .. t_max - 1, the Q of past rows, the gaps of the spread layout — is NaN, so a read
    outside shows up as NaN in the output, not as a small error.
    kind 'random': K, q, V standard normal, logits of order 1. The other two kinds carry logits of 120 (q and K scaled per head, each
    by the same factor; an unshifted exp overflows fp32 from 88.7 on) on answers that do not hinge on the last digits of an fp32
    logit, whose spacing at 120 is 7.6e-6: 'dominant': one key's logit is 120 and the others lie at least 60 below (p = 1 to 26
    digits); 'uniform': every key row is the same, so all logits are equal and the answer is the mean of the value rows."""
    g = torch.Generator().manual_seed(seed)
    D = H * dh
    ld, k_off, q_off, v_off = attn_layout(D, layout)
    t_max = n_keys + t_pad
    K = torch.randn(B, n_keys, H, dh, generator=g, dtype=torch.float64)
    V = torch.randn(B, n_keys, H, dh, generator=g, dtype=torch.float64)
    q = torch.randn(B, H, dh, generator=g, dtype=torch.float64)
    if kind == "uniform":
        K = K[:, :1].expand(B, n_keys, H, dh).clone()
    if kind == "dominant":  # the key at n_keys // 2 is 2 q / |q|, the others are scaled to |k| <= 1: cosines cannot reach it
        K = K / K.norm(dim=-1, keepdim=True).clamp_min(1.0)
        K[:, n_keys // 2] = 2.0 * q / q.norm(dim=-1, keepdim=True)
    if kind != "random":
        lg = torch.einsum("bkhd,bhd->bhk", K, q) / np.sqrt(dh)
        f = torch.sqrt(120.0 / lg.abs().amax(-1))  # [B, H]
        q, K = q * f[:, :, None], K * f[:, None, :, None]
    cache = torch.full((B, t_max, ld), float("nan"), dtype=dtype)
    cache[:, :n_keys, k_off:k_off + D] = K.reshape(B, n_keys, D).to(dtype)
    cache[:, :n_keys, v_off:v_off + D] = V.reshape(B, n_keys, D).to(dtype)
    cache[:, n_keys - 1, q_off:q_off + D] = q.reshape(B, D).to(dtype)
    return cache, (ld, k_off, q_off, v_off)


def attn_parts(cache, n_keys, H, dh, k_off, q_off, v_off):
    """the stored 16-bit values as fp64: K, V [B, n, H, dh], q [B, H, dh]"""
    B, D = cache.shape[0], H * dh
    c = cache[:, :n_keys].double()
    K = c[:, :, k_off:k_off + D].reshape(B, n_keys, H, dh)
    V = c[:, :, v_off:v_off + D].reshape(B, n_keys, H, dh)
    q = c[:, n_keys - 1, q_off:q_off + D].reshape(B, H, dh)
    return K, V, q


def attn_logits(cache, n_keys, H, dh, k_off, q_off, v_off):
    K, _, q = attn_parts(cache, n_keys, H, dh, k_off, q_off, v_off)
    return torch.einsum("bkhd,bhd->bhk", K, q) / np.sqrt(dh)


def attn_decode_ref(cache, n_keys, H, dh, k_off, q_off, v_off, mode):
    """mode 0: sum of the first n_keys value rows; mode 1: softmax over the keys of K[k].q / sqrt(dh), times V. fp64 -> [B, H dh]"""
    K, V, q = attn_parts(cache, n_keys, H, dh, k_off, q_off, v_off)
    if mode == 0:
        out = V.sum(1)
    else:
        p = torch.softmax(torch.einsum("bkhd,bhd->bhk", K, q) / np.sqrt(dh), -1)
        out = torch.einsum("bhk,bkhd->bhd", p, V)
    return out.reshape(cache.shape[0], H * dh)


def attn_decode_tol(ref, cache, n_keys, H, dh, v_off, mode):
    """|got - ref| <= u_out |ref| + c n_keys 2^-23 max|V|: the kernel accumulates in fp32 and rounds ONCE to the output type.
    u_out = 2^-8 (bf16) / 2^-11 (fp16) is one ulp of the output relative to a value at the bottom of its binade, where half an ulp is
    the final rounding itself; n_keys 2^-23 max|V| is the worst case of an fp32 sum of n_keys terms of size max|V| (max over the head's
    own value rows). c = 1 in mode 0; c = 2 in mode 1, which adds the error of __expf and of the fp32 logits to the same sum.
    (That doubling covers fp32 logits of order 1, and logits of any size where one key holds the weight or all are equal — the three
    kinds of attn_case. It does not cover a softmax that mixes keys at logits of 120, where an fp32 logit is only good to 1e-5: such
    inputs are not generated.)"""
    B, D = cache.shape[0], H * dh
    vmax = cache[:, :n_keys, v_off:v_off + D].double().abs().reshape(B, n_keys, H, dh).amax(dim=(1, 3))  # [B, H]
    vmax = vmax[:, :, None].expand(B, H, dh).reshape(B, D)
    return U_OUT[cache.dtype] * ref.abs() + (1 if mode == 0 else 2) * n_keys * 2.0 ** -23 * vmax


# ------------------------------------------------------------------------------------------------ mst_beam_step
BEAM_SIZES = ((1, 293), (4, 293), (7, 293), (16, 293), (16, 128), (16, 129), (4, 3), (16, 1))  # (K, V); K V <= 2048: scores in registers
BEAM_L = 514       # positions of a token row: 2 (T + 1) at T = 256; the row copy walks 256 columns at a time
REL_GAP = 1e-4     # a thousand times what fp32 logf and one fp32 subtraction can move a score (2^-23 = 1.2e-7)
LD_PAD = 5         # pad columns of the probability buffer: they hold 1.0 and would win if read


def beam_scores(probs, scores_in, seqs_in, i, K, eos=EOS, pad=PAD):
    """fp64 score of every candidate: [B, K V]; candidate c = k V + w continues hypothesis k with word w"""
    probs, scores_in = np.asarray(probs, np.float64), np.asarray(scores_in, np.float64)
    N, V = probs.shape
    last = np.asarray(seqs_in)[:, i - 1]
    fin = (last == eos) | ((last == pad) & (i > 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        cand = scores_in[:, None] - np.log(np.maximum(probs, 1e-30))  # (np.maximum passes a NaN on)
    done = np.full((N, V), np.inf)
    if pad < V:
        done[:, pad] = scores_in
    cand = np.where(fin[:, None], done, cand)
    cand = np.where(np.isnan(cand), np.inf, cand)
    return cand.reshape(N // K, K * V)


def beam_step_ref(probs, scores_in, seqs_in, i, K, eos=EOS, pad=PAD):
    """One position of beam search as the stable argsort it is documented to be. -> dict of seqs (first i + 1 columns), scores, hyp_src
    (global source row), word, alive (what the position adds to active[i])"""
    probs = np.asarray(probs)
    N, V = probs.shape
    B = N // K
    cand = beam_scores(probs, scores_in, seqs_in, i, K, eos, pad)
    top = np.argsort(cand, axis=1, kind="stable")[:, :K]
    hyp = (top // V + np.arange(B)[:, None] * K).reshape(-1)
    word = (top % V).reshape(-1)
    seqs = np.concatenate([np.asarray(seqs_in)[hyp, :i], word[:, None]], 1)
    return {"seqs": seqs.astype(np.int64), "scores": np.take_along_axis(cand, top, 1).reshape(-1), "hyp_src": hyp.astype(np.int64),
            "word": word.astype(np.int64), "alive": int(((word != eos) & (word != pad)).sum())}


def beam_min_gap(probs, scores_in, seqs_in, i, K, eos=EOS, pad=PAD):
    """per sample, the smallest relative difference between two neighbours among the reference's best 2 K FINITE scores (the ones that
    decide the selection and its order, the K-th against the (K + 1)-th included); inf where fewer than two are finite. Infinite
    candidates are bit-identical on the device too (NaN and a finished hypothesis's other words map to +inf there as here)."""
    cand = np.sort(beam_scores(probs, scores_in, seqs_in, i, K, eos, pad), axis=1)[:, :2 * K]
    a, b = cand[:, :-1], cand[:, 1:]
    with np.errstate(invalid="ignore"):
        rel = np.where(np.isfinite(b), (b - a) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300), np.inf)
    return rel.min(axis=1) if rel.shape[1] else np.full(cand.shape[0], np.inf)


def _draw_sample(rng, K, V, spec):
    """probabilities [K, V] fp32 (rows sum to 1, every entry >= 1e-6 / V) and non-negative scores [K] fp32, as beam search holds them"""
    p = rng.random((K, V)) ** 3 + 1e-6
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    s = (rng.random(K) * 40.0).astype(np.float32)
    if spec is not None:
        p, s = spec(rng, p, s)
    return p, s


def beam_separated_case(B, K, V, i, seed, L=BEAM_L, last=None, spec=None, max_rounds=200):
    """Inputs whose reference order is unambiguous: every sample is re-drawn until beam_min_gap >= REL_GAP (no sample is dropped; the
    caller asserts the gap). last: [B K] tokens of column i - 1 (default: live tokens); spec(rng, p, s) -> (p, s) edits a drawn sample
    (non-finite entries and the like) before it is judged. The token rows hold ids from [3, 300) whatever V is: the kernel copies
    them and compares column i - 1 with EOS and PAD, nothing else."""
    rng = np.random.default_rng(seed)
    seqs = rng.integers(3, 300, size=(B * K, L)).astype(np.int32)
    seqs[:, i:] = PAD
    if last is not None:
        seqs[:, i - 1] = last
    probs = np.zeros((B * K, V), np.float32)
    scores = np.zeros(B * K, np.float32)
    for b in range(B):
        rows = slice(b * K, (b + 1) * K)
        for _ in range(max_rounds):
            probs[rows], scores[rows] = _draw_sample(rng, K, V, spec)
            if beam_min_gap(probs[rows], scores[rows], seqs[rows], i, K)[0] >= REL_GAP:
                break
        else:
            raise RuntimeError(f"no separated draw for sample {b} in {max_rounds} rounds")
    return probs, scores, seqs


TIE_LEVELS = np.exp(-(1.0 + 0.37 * np.arange(6))).astype(np.float32)  # -log p = 1, 1.37, ...: neighbours 0.37 apart


def beam_tie_case(B, K, V, i, seed, L=BEAM_L, first_position=False):
    """Exact ties: every hypothesis of a sample holds the same score and every probability is one of six values whose logarithms lie
    0.37 apart, so two candidates either have the same fp32 inputs — and then the same score on the device whatever logf returns — or
    differ by 0.37. Hypotheses 0 and 1 hold the same row. first_position: column 0 is SOS, hypothesis 0 starts at 0 and the others at
    +inf, as decode.BeamSearch sets position 1 up (i must be 1)."""
    rng = np.random.default_rng(seed)
    seqs = rng.integers(3, 300, size=(B * K, L)).astype(np.int32)
    seqs[:, i:] = PAD
    probs = TIE_LEVELS[rng.integers(0, len(TIE_LEVELS), size=(B * K, V))]
    for b in range(B):
        if K > 1:
            probs[b * K + 1] = probs[b * K]
    scores = np.repeat((rng.random(B) * 40.0).astype(np.float32), K)
    if first_position:
        assert i == 1
        seqs[:, 0] = SOS
        scores = np.full((B, K), np.inf, np.float32)
        scores[:, 0] = 0.0
        scores = scores.reshape(-1)
    return probs, scores, seqs


def beam_ties_are_exact(probs, scores_in, seqs_in, i, K):
    """what beam_tie_case promises, checked on the reference's best 2 K: two neighbours are equal (same score in, same probability bits)
    or at least REL_GAP apart"""
    cand = np.sort(beam_scores(probs, scores_in, seqs_in, i, K), axis=1)[:, :2 * K]
    a, b = cand[:, :-1], cand[:, 1:]
    with np.errstate(invalid="ignore"):
        ok = (a == b) | ~np.isfinite(b) | ((b - a) >= REL_GAP * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


def beam_step_bruteforce(probs, scores_in, seqs_in, i, K, eos=EOS, pad=PAD):
    """beam_step_ref once more as a per-sample Python loop with an explicit (score, index) sort: what keeps the vectorised form honest"""
    probs = np.asarray(probs)
    N, V = probs.shape
    out = {"seqs": [], "scores": [], "hyp_src": [], "word": [], "alive": 0}
    for b in range(N // K):
        cands = []
        for k in range(K):
            h = b * K + k
            last = int(seqs_in[h][i - 1])
            fin = last == eos or (last == pad and i > 1)
            for w in range(V):
                if fin:
                    s = float(scores_in[h]) if w == pad else float("inf")
                else:
                    p = float(probs[h][w])
                    s = float(scores_in[h]) - float(np.log(max(p, 1e-30))) if p == p else float("nan")
                if s != s:
                    s = float("inf")
                cands.append((s, k * V + w))
        cands.sort()  # tuples: by score, then by index
        for s, c in cands[:K]:
            k, w = divmod(c, V)
            out["seqs"].append(list(seqs_in[b * K + k][:i]) + [w])
            out["scores"].append(s)
            out["hyp_src"].append(b * K + k)
            out["word"].append(w)
            out["alive"] += int(w != eos and w != pad)
    return {k: (np.asarray(v) if k != "alive" else v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ a long teacher-forced decode
LONG_N, LONG_B = 130, 4  # positions fed (past two waves of cached rows) and samples
LONG_DIMS = {"token": (40, 40, 2, 16, 64, 1, 2, 128, 1, 4), "pianoroll": (48, 48, 2, 16, 64, 1, 2, 128, 1, 4)}  # decoder 128 x 4 heads: dh = 32
# (mean, max) |dp| of the fp32 oracle on bf16-rounded weights against the fp32 oracle on fp32 weights over the LONG_N positions
# (storage_cost below; tests/test_decode_refs_cpu.py re-measures them): what 16-bit storage alone costs at this length.
STORAGE_COST = {("token", "query"): (8.54e-5, 1.66e-3), ("token", "key"): (1.17e-4, 4.41e-3),
                ("pianoroll", "query"): (6.98e-4, 3.80e-3), ("pianoroll", "key"): (1.15e-3, 1.79e-2)}


def long_decode_inputs(kind, seed=3):
    """-> (oracle module, its config, fp32 parameters, z [B, Z], classes [B], fed [B, n] tokens or [B, n, P] frames): the inputs of
    test_decode_step_matches_the_oracle's method at LONG_N positions (non-trivial biases and LayerNorm parameters)"""
    from oracle import vae_oracle as O
    dims = LONG_DIMS[kind]
    rng = np.random.default_rng(seed)
    ocfg = O.OracleConfig(kind, *dims)
    params = O.init_params(ocfg, rng)
    for k, v in params.items():
        if k.endswith("bias") or k.endswith("beta"):
            params[k] = (0.05 * rng.standard_normal(v.shape)).astype(np.float32)
        if k.endswith("gamma"):
            params[k] = (1.0 + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    z = rng.standard_normal((LONG_B, dims[3])).astype(np.float32)
    classes = rng.integers(0, 2, size=LONG_B)
    fed = rng.integers(1, dims[0], size=(LONG_B, LONG_N)) if kind == "token" else (rng.random((LONG_B, LONG_N, dims[0])) < 0.1).astype(np.uint8)
    return O, ocfg, params, z, classes, fed


def long_decode_oracle(O, ocfg, params, z, classes, fed, attention):
    P = O.to_torch_params(params, requires_grad=False)
    return O.decode_incremental(P, ocfg, torch.from_numpy(z), torch.from_numpy(classes), torch.from_numpy(fed), attention).numpy()


def storage_cost(kind, attention):
    """(mean, max) |dp| between the fp32 oracle on weights rounded to bf16 (every '.weight': the matrices and embedding tables, which
    the library keeps as 16-bit shadows) and the same oracle on the fp32 weights: what 16-bit storage alone costs at LONG_N positions"""
    O, ocfg, params, z, classes, fed = long_decode_inputs(kind)
    want = long_decode_oracle(O, ocfg, params, z, classes, fed, attention)
    rounded = {k: (torch.from_numpy(v).to(torch.bfloat16).float().numpy() if k.endswith("weight") else v) for k, v in params.items()}
    err = np.abs(long_decode_oracle(O, ocfg, rounded, z, classes, fed, attention) - want)
    return float(err.mean()), float(err.max())
