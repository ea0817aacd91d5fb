"""mst_kqv_ffn_ln_bwd on a real MI355X: the K | Q | V input gradient as the head of the feed-forward backward launch against the two
launches it replaces (mst_gemm_nt, then mst_ffn_ln_bwd_lead on its result), on identical inputs, bit for bit — the gradient tile itself
(stored only on request), the leading LayerNorm backward's dx and masked copy, d(pre), the block's dx and masked copy, the LayerNorm
partial rows; with atomics instead of partial rows the parameter gradients within the rounding of an fp32 sum in another order. Every
output lies in a sentinel-filled buffer with guard rows and pad columns, which both runs must leave alone. Then the step: two encoder
layers, two steps, with and without the head — every gradient and every weight bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

GUARD, PAD = 70, 8           # guard rows behind a buffer's M rows (more than a tile's 64: a ragged tile's missing rows are among them)
SENT16, SENT32 = 0x7F7F, 0x7F7F7F7F
SITE_LEAD, SITE_LN1 = 5, 9
RAGGED = 17


def _inputs(dtype, D, M, dense, gpu):
    """operands of one case, made on the host from a fixed seed: the same for both runs"""
    g = torch.Generator().manual_seed(1000 * D + M + (7 if dense else 0))
    F = 4 * D
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale  # noqa: E731
    resid = r(M, D, scale=0.5)
    if not dense:  # the top layer's d(h1): zero outside each sample's position 0 — here every 13th row, and the last one
        keep = torch.zeros(M, dtype=torch.bool)
        keep[::13] = True
        keep[M - 1] = True
        resid[~keep] = 0.0
    x2, x1 = r(M, D) + 0.25, r(M, D) - 0.5
    ins = dict(dqkv=r(M, 3 * D, scale=0.25).to(dtype), Wt=r(D, 3 * D, scale=D ** -0.5).to(dtype), resid=resid.to(dtype),
               x2=x2.to(dtype), x1=x1.to(dtype), gate=torch.relu(r(M, F)).to(dtype), W2t=r(F, D, scale=D ** -0.5).to(dtype),
               W1t=r(D, F, scale=F ** -0.5).to(dtype), g2=1.0 + 0.1 * r(D), g1=1.0 + 0.1 * r(D),
               seed_word=torch.tensor([0x5EED5EED1234], dtype=torch.int64))
    for k, x in (("2", ins["x2"]), ("1", ins["x1"])):
        xf = x.float()
        ins["mean" + k] = xf.mean(1)
        ins["rstd" + k] = 1.0 / torch.sqrt(xf.var(1, unbiased=False) + 1e-5)
    return {k: t.to(gpu) for k, t in ins.items()}


def _outputs(dtype, D, M, tiles, gpu, parts):
    """sentinel-filled output buffers: [M + GUARD, width + PAD] 16-bit, the partial rows [tiles + 2, 2 D], the parameter gradients zero"""
    F = 4 * D
    b16 = lambda w: torch.full((M + GUARD, w + PAD), SENT16, dtype=torch.int16, device=gpu).view(dtype)  # noqa: E731
    u = dict(dy=b16(D), dh=b16(D), dhm=b16(D), dpre=b16(F), dh1=b16(D), dh1m=b16(D))
    for p in ("l_", ""):
        u[p + "dgamma"], u[p + "dbeta"] = torch.zeros(D, device=gpu), torch.zeros(D, device=gpu)
        u[p + "parts"] = torch.full((tiles + 2, 2 * D), SENT32, dtype=torch.int32, device=gpu).view(torch.float32) if parts else None
    return u


def _run(o, how, ins, u, D, M, p, ldr_odd=False):
    """how: 'two' — gemm_nt, then ffn_ln_bwd with the lead; 'head' — ffn_ln_bwd(head=) storing dy; 'head_nostore' — without C_out"""
    F = 4 * D
    v = lambda name, w=D: u[name][:M, :w]  # noqa: E731
    drop = lambda site: dict(dropout_p=p, dropout_seed=77, dropout_seed_ptr=ins["seed_word"], dropout_site=site) if p > 0 else {}  # noqa: E731
    resid = ins["resid"]
    if ldr_odd:  # a residual whose leading dimension is a multiple of 4, not of 8: mst_gemm_nt takes it, the head's 16-byte loads do not
        wide = torch.zeros(M, D + 4, dtype=resid.dtype, device=resid.device)
        wide[:, :D] = resid
        resid = wide[:, :D]
    gemm = dict(A=ins["dqkv"], B=ins["Wt"], resid=resid, N=D, K=3 * D)
    lead = dict(x=ins["x2"], gamma=ins["g2"], mean=ins["mean2"], rstd=ins["rstd2"], dx=v("dh"), dx_masked=v("dhm") if p > 0 else None,
                dgamma=u["l_dgamma"], dbeta=u["l_dbeta"], partials=u["l_parts"], **drop(SITE_LEAD))
    dff = v("dhm") if p > 0 else v("dh")
    kw = dict(alpha=1.0 / (1.0 - p) if p > 0 else 1.0, dx_masked=v("dh1m") if p > 0 else None, mask_mode=1 if p > 0 else 0,
              partials=u["parts"], resid=v("dh"), K=F, **drop(SITE_LN1))
    args = (dff, ins["W2t"], v("dpre", F), ins["gate"], ins["W1t"], v("dh1"), ins["x1"], ins["g1"], ins["mean1"], ins["rstd1"], u["dgamma"], u["dbeta"])
    if how == "two":
        o.gemm_nt(gemm["A"], gemm["B"], v("dy"), resid=resid, N=D, K=3 * D)
        o.ffn_ln_bwd(*args, lead=dict(lead, dy=v("dy")), **kw)
    else:
        o.ffn_ln_bwd(*args, lead=lead, head=dict(gemm, C_out=v("dy") if how == "head" else None), **kw)
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()  # noqa: E731
    return {k: bits(t) for k, t in u.items() if t is not None}


def _same_bits(got, want, M, tiles, skip=()):
    for k in want:
        if k in skip or k.endswith("dgamma") or k.endswith("dbeta"):
            continue
        a, b = got[k], want[k]
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{k}: {len(bad)} elements differ, first at {bad[0].tolist()} (rows >= {M} / partial rows >= {tiles} are guards)"


def _guards_intact(out, M, tiles):
    for k, a in out.items():
        if a.dtype == np.int16:
            w = a.shape[1] - PAD
            assert (a[M:] == SENT16).all() and (a[:, w:] == SENT16).all(), f"{k}: a guard row or pad column was written"
        elif k.endswith("parts"):
            assert (a[tiles:] == SENT32).all(), f"{k}: a partial row past the launch's {tiles} workgroups was written"


CASES = [(D, dt, tiles, ragged, dense, p)
         for D in (256, 128) for dt in (torch.bfloat16, torch.float16)
         for tiles, ragged in ((28, False), (8, False), (3, False), (28, True))
         for dense, p in ((False, 0.0), (False, 0.1), (True, 0.1))]


@pytest.mark.parametrize("D,dtype,tiles,ragged,dense,p", CASES,
                         ids=lambda x: {torch.bfloat16: "bf16", torch.float16: "fp16"}.get(x, str(x)))
def test_head_against_the_two_launches_bit_for_bit(gpu, D, dtype, tiles, ragged, dense, p):
    """28 tiles reach every chunk rotation (blockIdx.x / 8) % 4, 8 are one round of the eight XCDs, 3 are short of one; the ragged M
    takes the guarded kernel form"""
    from musicstyletransfer_amd import ops as o
    M = tiles * 64 - (RAGGED if ragged else 0)
    ins = _inputs(dtype, D, M, dense, gpu)
    head = dict(A=ins["dqkv"], B=ins["Wt"], resid=ins["resid"], N=D, K=3 * D)
    probe = _outputs(dtype, D, M, tiles, gpu, True)
    assert o.ffn_ln_bwd_head_form(head, probe["dh"][:M, :D], ins["W2t"], probe["dpre"][:M, :4 * D], ins["gate"], ins["W1t"],
                                  probe["dh1"][:M, :D]) == 1
    assert o.gemm_nt_ln_parts(M) == tiles
    want = _run(o, "two", ins, _outputs(dtype, D, M, tiles, gpu, True), D, M, p)
    got = _run(o, "head", ins, _outputs(dtype, D, M, tiles, gpu, True), D, M, p)
    unused = () if p > 0 else ("dhm", "dh1m")
    _guards_intact(want, M, tiles)
    _guards_intact(got, M, tiles)
    _same_bits(got, want, M, tiles)
    for k in unused:
        assert (got[k] == SENT16).all()
    # the gradient tile is stored on request only; everything else is the same without it
    nostore = _run(o, "head_nostore", ins, _outputs(dtype, D, M, tiles, gpu, True), D, M, p)
    assert (nostore["dy"] == SENT16).all()
    _same_bits(nostore, want, M, tiles, skip=("dy",))
    _guards_intact(nostore, M, tiles)
    assert (want["dy"][:M, :D] != SENT16).any() and np.abs(want["dh1"][:M, :D].astype(np.int32)).max() > 0


@pytest.mark.parametrize("D", (256, 128))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
def test_parameter_gradients_by_atomics(gpu, D, dtype):
    """without a partials buffer each workgroup adds its column sums with fp32 atomics, in no fixed order: both forms must lie within
    tiles * 2^-24 * sum |partial rows| of the exact sum of the partial rows — above gamma_(tiles - 1) sum |x|, the bound of an fp32 sum
    of `tiles` terms in any order — and the partial rows themselves are bit-identical between the forms (the test above)"""
    from musicstyletransfer_amd import ops as o
    tiles, p = 28, 0.1
    M = tiles * 64
    ins = _inputs(dtype, D, M, True, gpu)
    rows = _run(o, "head", ins, _outputs(dtype, D, M, tiles, gpu, True), D, M, p)
    for how in ("two", "head"):
        out = _run(o, how, ins, _outputs(dtype, D, M, tiles, gpu, False), D, M, p)
        for pre in ("l_", ""):
            parts = rows[pre + "parts"][:tiles].view(np.float32).astype(np.float64)
            exact, mass = parts.sum(0), np.abs(parts).sum(0)
            got = np.concatenate([out[pre + "dgamma"].view(np.float32), out[pre + "dbeta"].view(np.float32)]).astype(np.float64)
            err = np.abs(got - exact)
            bound = tiles * 2.0 ** -24 * mass + 2.0 ** -149
            assert (err <= bound).all(), f"{how} {pre}dgamma|dbeta: worst {float((err / bound).max()):.3g} of the bound"


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
def test_a_shape_the_form_refuses_runs_the_two_launches(gpu, dtype):
    """a residual with a leading dimension that is no multiple of 8: the call issues mst_gemm_nt itself, then the launch with the lead"""
    from musicstyletransfer_amd import ops as o
    D, tiles, p = 256, 3, 0.1
    M = tiles * 64
    ins = _inputs(dtype, D, M, False, gpu)
    wide = torch.zeros(M, D + 4, dtype=dtype, device=gpu)
    probe = _outputs(dtype, D, M, tiles, gpu, True)
    assert o.ffn_ln_bwd_head_form(dict(A=ins["dqkv"], B=ins["Wt"], resid=wide[:, :D], N=D, K=3 * D), probe["dh"][:M, :D], ins["W2t"],
                                  probe["dpre"][:M, :4 * D], ins["gate"], ins["W1t"], probe["dh1"][:M, :D]) == 0
    want = _run(o, "two", ins, _outputs(dtype, D, M, tiles, gpu, True), D, M, p)
    got = _run(o, "head", ins, _outputs(dtype, D, M, tiles, gpu, True), D, M, p, ldr_odd=True)
    _same_bits(got, want, M, tiles)
    _guards_intact(got, M, tiles)


def test_two_steps_with_and_without_the_head(gpu):
    """two encoder layers at B 4, T 64 (four tiles), dropout on: the step's launches with Forms.kqv_head_e off and on.
    With four workgroups per LayerNorm-backward launch the step keeps the fp32 atomics for the LayerNorm parameter gradients
    (StepPlan.LN_PARTIALS_MIN = 32 workgroups), and then two runs of ONE form already differ in them: measured here, head off against
    head off, 125 of 256 entries of encoder.layer0.ln1.gamma's gradient by up to 4.8e-7 at scale 8.2 (ln1.beta, ln2.gamma, ln2.beta and
    the decoder's likewise), every other gradient and every activation gradient equal. Both plans therefore take the partial rows at
    this size too (LN_PARTIALS_MIN = 1: the deterministic form the step uses from 32 tiles on), and every gradient and weight must match."""
    from musicstyletransfer_amd import engine as E
    from oracle import vae_oracle as O
    dims = ("pianoroll", 128, 128, 2, 16, 256, 2, 8, 64, 1, 4)
    B, T = 4, 64
    rng = np.random.default_rng(3)
    ocfg = O.OracleConfig(*dims)
    params = O.init_params(ocfg, rng)
    batch = O.synthetic_pianoroll_batch(rng, B, T, 128)
    eps = rng.standard_normal((B, dims[4])).astype(np.float32)
    res = {}
    for on in (False, True):
        cfg = E.VAEConfig(*dims, e_dropout=0.1, d_dropout=0.1)
        store = E.ParamStore(cfg, gpu, torch.bfloat16, params_np=params)
        plan = E.StepPlan(store, B, T, lr=1e-3)
        plan.kqv_head = on
        plan.LN_PARTIALS_MIN = 1
        grads = []
        for _ in range(2):
            plan.load_batch(batch["x"], batch["seq_lens"], batch["classes"], batch["labels"], eps)
            plan.step_kernels(True)
            torch.cuda.synchronize()
            assert plan.forms.kqv_head_e == on
            grads.append(store.g.clone())
        res[on] = (grads, store.w.clone())
    for step in range(2):
        assert torch.equal(res[False][0][step].view(torch.int32), res[True][0][step].view(torch.int32)), f"gradients of step {step + 1} differ"
    assert torch.equal(res[False][1].view(torch.int32), res[True][1].view(torch.int32)), "weights after two steps differ"
    assert float(res[True][0][1].abs().max()) > 0
