"""tests/loss_refs.py without a GPU: the fp64 references against torch autograd, the fp32-ordered branch against the oracle, the case
tables against the library's own launch decisions (mst_sigmoid_bce_form / mst_gemm_sigmoid_bce_form) and their edges, and the derived
tolerances — they accept an fp32 emulation that rounds where the kernels round, in two summation orders, and refuse every wrong
kernel listed in loss_refs.BCE_MISTAKES / CE_MISTAKES wherever the mistake changes a result."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import loss_refs as L  # noqa: E402

BF, FP = L.BF, L.FP
BCE_RUNS = [(c, d, m) for c in L.BCE_CASES for d in L.DTYPES for m in c.modes]
FUSED_RUNS = [(c, d, m) for c in L.FUSED_CASES for d in L.DTYPES for m in c.modes]
CE_RUNS = [(c, d, m) for c in L.CE_CASES for d in L.DTYPES for m in c.modes]
_id = lambda r: f"{r[0].id}-{L.DT_NAME[r[1]]}-{r[2]}"  # noqa: E731


@pytest.fixture(scope="module")
def ops():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib, ops as o
    _lib.load()
    return o


def _bce_xy(c, dtype, mode):
    o = L.bce_operands(c.id, dtype, mode)
    x = o["logits"][:, :c.P].double().numpy().reshape(c.B, c.T, c.P)
    return x, o["labels"].numpy().reshape(c.B, c.T, c.P)


def _fused_xy(c, dtype, mode):
    """the logits a correct launch stores (the fp64 GEMM rounded to the type) and the labels"""
    o = L.fused_operands(c.id, dtype, mode)
    ref, _ = L.fused_logits_ref(c, o, dtype)
    return L.round_to(ref, dtype).reshape(c.B, c.T, c.P), o["labels"].numpy().reshape(c.B, c.T, c.P)


# ------------------------------------------------------------------------------------------ the references themselves
def _torch_bce(x, labels, ls, dw, gscale, dt=torch.float64):
    """loss.py:27-80 restated with torch autograd"""
    B = x.shape[0]
    xt = torch.tensor(x, dtype=dt, requires_grad=True)
    y = torch.tensor(labels, dtype=dt)
    ls = float(np.float32(ls))
    p = torch.sigmoid(xt)
    omp = torch.sigmoid(-xt) if dt == torch.float64 else 1.0 - p
    s = (1.0 - ls) * y + 0.5 * ls
    bce = -(s * torch.log(1e-12 + p) + (1.0 - s) * torch.log(1e-12 + omp))
    if dw:
        y2 = y.reshape(B, -1)
        w = ((y2 == 1).sum(1).to(dt) / ((y2 != 1).sum(1).to(dt) + 1e-12)).reshape(B, 1, 1)
        bce = torch.where(y == 0, (w * bce) * bce, bce)
    loss = bce.reshape(B, -1).mean(1)
    (loss.sum() * float(np.float32(gscale))).backward()
    return p.detach().numpy(), xt.grad.numpy(), loss.detach().numpy()


@pytest.mark.parametrize("run", BCE_RUNS, ids=_id)
def test_bce_reference_equals_torch_autograd_in_fp64(run):
    """every element at or below 9 (beyond it the reference value is the fp32-stepped one); the loss where a sample has no such element"""
    c, dtype, mode = run
    x, labels = _bce_xy(c, dtype, mode)
    r = L.bce_references(c.id, dtype, mode)
    p, g, loss = _torch_bce(x, labels, c.ls, c.dw, c.gscale)
    keep = ~r["sat"]
    assert np.allclose(r["probs"][keep], p[keep], rtol=1e-12, atol=0)
    # (torch's sigmoid backward forms 1 - sigmoid(-x), which cancels to 0 below -37: an absolute 1.1e-16 on that factor)
    assert np.allclose(r["dlogits"][keep], g[keep], rtol=1e-9, atol=4e-16 * c.gscale / (c.T * c.P))
    clean = ~r["sat"].reshape(c.B, -1).any(1)
    assert np.allclose(r["loss"][clean], loss[clean], rtol=1e-12, atol=0)
    assert np.array_equal(r["npos"], labels.reshape(c.B, -1).sum(1))
    assert mode == "sat" or clean.all()


@pytest.mark.parametrize("ls,dw", [(0.0, False), (0.1, False), (0.0, True), (0.1, True)])
def test_the_fp32_ordered_branch_equals_the_oracle_on_saturated_logits(ls, dw):
    from vae_oracle import binary_cross_entropy
    rng = np.random.default_rng(5)
    B, n = 3, 400
    x = rng.choice(L.SAT_HI + L.SAT_LO + (12.0, 14.5, 16.0, -17.0, -20.0), (B, n))
    y = (rng.random((B, n)) < 0.2).astype(np.uint8)
    npos = y.sum(1).astype(np.float32)
    w = (npos / ((np.float32(n) - npos) + np.float32(1e-12))).astype(np.float32).reshape(B, 1)
    _, bce, _ = L.exact32(x, y, ls, w, dw)
    want = binary_cross_entropy(torch.tensor(x, dtype=torch.float32), torch.tensor(y), label_smoothing=ls, negative_label_downweighting=dw)
    got = bce.astype(np.float64).mean(1)
    assert np.allclose(got, want.double().numpy(), rtol=2e-6, atol=0)
    # the oracle's fp32 gradient too, element by element, where p is exactly 1 or 1 - p exactly 1 (its autograd takes another route between)
    xt = torch.tensor(x, dtype=torch.float32, requires_grad=True)
    binary_cross_entropy(xt, torch.tensor(y), label_smoothing=ls, negative_label_downweighting=dw).sum().backward()
    _, _, d = L.exact32(x, y, ls, w, dw)
    flat = x >= 17.5
    assert np.array_equal(d[flat], np.zeros(int(flat.sum()), dtype=np.float32)) and not xt.grad.numpy()[flat].any()


def _torch_ce(x, labels, c):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lab = torch.tensor(labels, dtype=torch.int64)
    p = torch.softmax(xt, -1)
    nll = -torch.log_softmax(xt, -1).gather(1, lab.view(-1, 1)).squeeze(1) * (lab != 0)
    loss = nll.view(c.B, c.T).mean(1)
    (loss.sum() * float(np.float32(c.gscale))).backward()
    return p.detach().numpy(), xt.grad.numpy(), loss.detach().numpy()


@pytest.mark.parametrize("run", [r for r in CE_RUNS if r[1] == BF], ids=_id)
def test_ce_reference_equals_torch_autograd_in_fp64(run):
    c, dtype, mode = run
    o = L.ce_operands(c.id, dtype, mode)
    x, labels = o["logits"][:, :c.V].double().numpy(), o["labels"].numpy().astype(np.int64)
    r = L.ce_references(c.id, dtype, mode)
    p, g, loss = _torch_ce(x, labels, c)
    assert np.allclose(r["probs"], p, rtol=1e-10, atol=1e-300)
    assert np.allclose(r["dlogits"], g, rtol=1e-9, atol=1e-18)
    assert np.allclose(r["loss"], loss, rtol=1e-12, atol=1e-15)
    # the token metrics against argmax / topk of the 16-bit values, where no tie touches the label
    tv = labels != 0
    assert r["tok"][3] == tv.sum()
    if mode != "known":   # (rows in which another entry equals the label's are left to the tie tests: topk's choice among ties is its own)
        xt = torch.tensor(x)
        lone = (x == x[np.arange(c.M), labels][:, None]).sum(1) == 1
        beat = (x > x[np.arange(c.M), labels][:, None]).sum(1)
        tied = tv & ~lone
        top = (xt.topk(min(c.top_k, c.V), dim=1).indices.numpy() == labels[:, None]).any(1)
        lo = int(((xt.argmax(1).numpy() == labels) & tv & lone).sum()), int((top & tv & lone).sum())
        assert lo[0] <= r["tok"][1] <= lo[0] + int((tied & (beat == 0)).sum())
        assert lo[1] <= r["tok"][2] <= lo[1] + int(tied.sum())
        assert tied.any() or (r["tok"][1], r["tok"][2]) == lo


def test_the_tie_rule_by_hand():
    """V = 6, label 3 with value 1: equal entries at 1 and 4, a larger one at 5 -> beaten by index 1 (equal, lower index) and 5: rank 2"""
    c = L.CeCase("hand", 1, 1, 6, 8, 8, top_k=2)
    x = np.array([[0.0, 1.0, -1.0, 1.0, 1.0, 2.0]])
    lab = np.array([3])
    assert L.ce_ref(x, lab, c, BF)["tok"][1:].tolist() == [0.0, 0.0, 1.0]                                   # beat = 2: not < 2
    assert L.ce_ref(x, lab, c, BF, mistake="topk_le", emulate=0)["tok"][2] == 1.0                           # 2 <= 2
    assert L.ce_ref(x, lab, L.CeCase("hand", 1, 1, 6, 8, 8, top_k=3), BF)["tok"][2] == 1.0
    assert L.ce_ref(x, lab, L.CeCase("hand", 1, 1, 6, 8, 8, top_k=3), BF, mistake="ties_to_higher", emulate=0)["tok"][2] == 1.0  # index 4, 5 beat it: 2
    x[0, 5] = 0.0   # only the ties are left: the lower index wins -> index 1 beats the label, rank 1
    assert L.ce_ref(x, lab, c, BF)["tok"][1:].tolist() == [0.0, 1.0, 1.0]
    assert L.ce_ref(x, np.array([1]), c, BF)["tok"][1] == 1.0        # the lowest of the tied entries IS the arg-max
    assert L.ce_ref(x, np.array([1]), c, BF, mistake="ties_to_higher", emulate=0)["tok"][1] == 0.0


def test_the_tie_case_really_holds_ties_around_the_label():
    c = L.CE_CASE["v37-ties"]
    for dtype in L.DTYPES:
        o = L.ce_operands(c.id, dtype, "real")
        x, lab = o["logits"][:, :c.V].double().numpy(), o["labels"].numpy()
        seen_lo = seen_hi = above = below = 0
        for m in range(c.M):
            if lab[m] == 0:
                continue
            eq = np.nonzero(x[m] == x[m, lab[m]])[0]
            seen_lo += int((eq < lab[m]).any())
            seen_hi += int((eq > lab[m]).any())
            step = 2.0 * L.half_ulp(x[m, lab[m]], dtype)
            above += int((np.abs(x[m] - (x[m, lab[m]] + step)) < step / 4).any())
            below += int((np.abs(x[m] - (x[m, lab[m]] - step)) < step / 4).any())
        assert min(seen_lo, seen_hi, above, below) >= 3
        assert L.ce_mistake_applies("ties_to_higher", x, lab.astype(np.int64), c)


# ------------------------------------------------------------------------------------------ the tables against the launch decisions
def test_abi_110_exports_the_form_queries(ops):
    from musicstyletransfer_amd import _lib
    assert _lib.load().mst_version() >= 110
    assert len(_lib.SIGNATURES["mst_sigmoid_bce_form"][1]) == len(_lib.SIGNATURES["mst_sigmoid_bce"][1]) == 18
    assert len(_lib.SIGNATURES["mst_gemm_sigmoid_bce_form"][1]) == 5


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: L.DT_NAME[d])
def test_every_bce_case_gets_its_form_and_the_table_reaches_every_value(ops, dtype):
    seen = [set() for _ in range(5)]
    for c in L.BCE_CASES:
        f = L.form_tuple(ops.sigmoid_bce_form(**L.bce_form_call(c, dtype)))
        assert f == c.form, f"{c.id}: meant for {c.form}, the launch takes {f}"
        for s, v in zip(seen, f):
            s.add(v)
    # count0 = 1 needs a labels base pointer off an 8-byte boundary, which no caller constructs (the issue's out of scope)
    assert seen[0] == {8, 4} and seen[1] == {8, 4, 1} and seen[2] == {0, 8} and seen[3] == {0, 8, 1} and seen[4] == {1, 2}


def _bce_form(ops, **over):
    c = L.BCE_CASE["p128-wide"]
    kw = L.bce_form_call(c, BF)
    kw.update(over)
    return ops.sigmoid_bce_form(**kw)


@pytest.mark.parametrize("over,vec,lab,why", [
    (dict(), 8, 8, "everything a multiple of 8, every pointer aligned"),
    (dict(ld_logits=132), 4, 4, "ld % 8 != 0"), (dict(ldp=132), 4, 4, "ldp % 8 != 0"), (dict(ldd=132), 4, 4, "ldd % 8 != 0"),
    (dict(probs=None, ldp=4), 8, 8, "an absent output's leading dimension is not looked at"),
    (dict(dlogits=None, ldd=0), 8, 8, "the same for dlogits"),
    (dict(logits=(1 << 20) + 8), 4, 4, "logits 8 bytes off"), (dict(probs=(5 << 20) + 8), 4, 4, "probs 8 bytes off"),
    (dict(dlogits=(6 << 20) + 8), 4, 4, "dlogits 8 bytes off"),
    (dict(P=124, ld_logits=128), 4, 4, "P % 8 != 0, P % 4 == 0"), (dict(P=126, ld_logits=128), 4, 1, "P % 4 != 0"),
])
def test_the_vector_width_at_its_edges(ops, over, vec, lab, why):
    f = _bce_form(ops, **over)
    assert (f["vec"], f["label_bytes"]) == (vec, lab), why


@pytest.mark.parametrize("B,T,P,gx,why", [
    (2, 64, 128, 2, "2048 four-pitch vectors: two workgroups of 1024"), (2, 32, 128, 1, "1024 vectors: one"), (2, 33, 128, 2, "1056: two"),
    (512, 64, 128, 1, "ceil(512 / B) = 1"), (511, 64, 128, 2, "ceil(512 / 511) = 2"), (600, 64, 128, 1, "B above 512"),
    (1, 4096, 128, 128, "131072 vectors: 128 workgroups, below ceil(512 / 1)"), (1, 1 << 16, 128, 512, "the cap of 512 / B"),
    (3, 7, 30, 1, "56 vectors"), (65535, 1, 4, 1, "the largest batch")])
def test_workgroups_per_sample_at_both_limits(ops, B, T, P, gx, why):
    assert _bce_form(ops, B=B, T=T, P=P, ld_logits=roundup4(P), ldp=roundup4(P), ldd=roundup4(P))["gx"] == gx, why


def roundup4(v):
    return L.roundup(v, 4)


@pytest.mark.parametrize("over,text", [
    (dict(B=0), b"must be positive"), (dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(loss=None), b"null pointer"),
    (dict(ld_logits=126), b"ld must be"), (dict(ld_logits=124), b"ld must be"), (dict(ldp=130), b"bad ldp"), (dict(ldd=64), b"bad ldd"),
    (dict(npos=None), b"npos scratch"), (dict(B=65536), b"grid.y"), (dict(T=1 << 27), b"below 2^31"),
])
def test_the_bce_form_query_refuses_what_the_launch_refuses(ops, over, text):
    """validation comes before any HIP call in both: same status, same message"""
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    kw = L.bce_form_call(L.BCE_CASE["p128-wide"], BF)
    kw.update(over)
    a = (0, kw["B"], kw["T"], kw["P"], kw["logits"], kw["ld_logits"], kw["labels"], kw["label_smoothing"], 1, kw["npos"], kw["loss"],
         kw["probs"], kw["ldp"], kw["dlogits"], kw["ldd"], kw["gscale"], 0)
    form = (ctypes.c_int64 * 8)()
    rc = lib.mst_sigmoid_bce_form(*a, form)
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg, (rc, msg)
    assert lib.mst_sigmoid_bce(*a, None) == -1 and lib.mst_last_error() == msg


def test_the_form_queries_refuse_an_unknown_type(ops):
    with pytest.raises(TypeError):
        ops.sigmoid_bce_form(**dict(L.bce_form_call(L.BCE_CASE["p128-wide"], BF), dtype=torch.float32))
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    kw = L.bce_form_call(L.BCE_CASE["p128-wide"], BF)
    form = (ctypes.c_int64 * 8)()
    rc = lib.mst_sigmoid_bce_form(7, kw["B"], kw["T"], kw["P"], kw["logits"], kw["ld_logits"], kw["labels"], 0.0, 1, kw["npos"], kw["loss"],
                                  kw["probs"], kw["ldp"], kw["dlogits"], kw["ldd"], 1.0, 0, form)
    assert rc == -3 and b"unsupported activation dtype" in lib.mst_last_error()
    g, q, _, _ = _fused_structs(L.FUSED_CASE["bn128"], BF, g__dtype=7)
    assert lib.mst_gemm_sigmoid_bce_form(ctypes.byref(g), ctypes.byref(q), None, None, (ctypes.c_int64 * 4)()) == -3


def _fused_structs(c, dtype, **over):
    """mst_gemm_args / mst_bce_args (/ the dgrad pair) of a fused case with dummy aligned pointers: for the form query, which follows none"""
    from musicstyletransfer_amd import _lib
    Pn, A = c.P, 1 << 20
    g = _lib.GemmArgs()
    g.dtype, g.M, g.N, g.K = (0 if dtype == BF else 1), c.M, Pn, c.K
    g.A, g.lda, g.B, g.ldb, g.bias, g.alpha = A, c.K, 2 * A, c.K, 3 * A, c.alpha
    g.C, g.ldc = (4 * A if c.with_c else None), (Pn + 8 if c.with_c else 0)
    g.a_rows_per_group, g.a_group_stride, g.a_group_offset = c.T, c.T + 1, 1
    q = _lib.BceArgs()
    q.labels, q.T, q.label_smoothing, q.downweight, q.loss, q.gscale = 5 * A, c.T, c.ls, int(c.dw), 6 * A, c.gscale
    q.probs, q.ldp = (7 * A if c.with_probs else None), (Pn + 8 if c.with_probs else 0)
    q.logits, q.ldl = 8 * A, Pn + 8
    g2 = l = None
    if c.dgrad:
        g2, l = _lib.GemmArgs(), _lib.LnArgs()
        g2.dtype, g2.M, g2.N, g2.K, g2.alpha = g.dtype, c.M, c.K, Pn, 1.0
        g2.A, g2.lda, g2.B, g2.ldb, g2.C, g2.ldc = g.C, g.ldc, 9 * A, Pn, 10 * A, c.K + 8
        g2.c_rows_per_group, g2.c_group_stride, g2.c_group_offset = c.T, c.T + 1, 1
        g2.dropout_p, g2.dropout_site, g2.dropout_seed_ptr = c.drop, L.FUSED_SITE, (11 * A if c.drop > 0 else None)
        l.mode, l.gamma, l.mean, l.rstd, l.x, l.ld_x, l.mask_mode, l.partials = 2, 12 * A, 13 * A, 14 * A, 15 * A, c.K, 2, 16 * A
        l.dgamma, l.dbeta = 17 * A, 18 * A
    for k, v in over.items():
        obj, name = k.split("__")
        setattr(dict(g=g, q=q, g2=g2, l=l)[obj], name, v)
    return g, q, g2, l


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: L.DT_NAME[d])
def test_every_fused_case_gets_its_form_and_the_table_reaches_every_value(ops, dtype):
    seen = [set() for _ in range(3)]
    for c in L.FUSED_CASES:
        f = ops.gemm_sigmoid_bce_form(*_fused_structs(c, dtype))
        f = (f["BN"], f["col_tiles"], f["launches"])
        assert f == c.form, f"{c.id}: meant for {c.form}, the launch takes {f}"
        for s, v in zip(seen, f):
            s.add(v)
    assert seen[0] == {128, 256} and seen[2] == {0, 1, 2} and {1, 2} <= seen[1]


def _LD(n):
    return dict(g__ldc=n + 8, q__ldp=n + 8, q__ldl=n + 8)


@pytest.mark.parametrize("cid,over,want,text", [
    ("bn128", dict(g__N=256, **_LD(256)), (256, 1, 0), None), ("bn128", dict(g__N=512, **_LD(512)), (256, 2, 0), None),
    ("bn128", dict(g__N=2048, **_LD(2048)), (256, 8, 0), None),
    ("bn128", dict(g__N=384, **_LD(384)), None, b"128 or a multiple of 256"), ("bn128", dict(g__N=64), None, b"128 or a multiple of 256"),
    ("bn256-dw", dict(), (256, 1, 0), None), ("bn256-dw", dict(g__N=512, **_LD(512)), None, b"down-weighting"),
    ("bn128", dict(q__T=96, g__M=192), None, b"multiple of 64"), ("bn128", dict(q__T=128), (128, 1, 0), None),
    ("bn128", dict(g__M=96), None, b"divide M"), ("bn128", dict(g__ldc=132), None, b"bad dlogits layout"),
    ("bn128", dict(q__labels=(5 << 20) + 4), None, b"8-byte aligned"), ("bn128", dict(g__A=(1 << 20) + 8), None, b"16-byte aligned"),
    ("bn128", dict(q__ldp=132), None, b"bad probs layout"), ("bn128", dict(q__ldl=100), None, b"bad logits layout"),
    ("bn128", dict(g__c_rows_per_group=64), None, b"only bias, alpha and an A row remap"),
    # _dgrad_ln: one launch only at 128 pitches, width 128, the second GEMM reading the first one's gradient
    ("dgrad-one", dict(), (128, 1, 1), None), ("dgrad-one", dict(g2__A=(4 << 20) + 16), (128, 1, 2), None),
    ("dgrad-one", dict(g2__lda=144), (128, 1, 2), None), ("dgrad-one", dict(g2__a_rows_per_group=64), (128, 1, 2), None),
    ("dgrad-two-p256", dict(), (256, 1, 2), None),
])
def test_the_fused_dispatch_at_its_edges(ops, cid, over, want, text):
    """the form query refuses what the launches refuse, with their message (validation precedes every HIP call in both)"""
    from musicstyletransfer_amd import _lib
    lib = _lib.load()
    g, q, g2, l = _fused_structs(L.FUSED_CASE[cid], BF, **over)
    if want is not None:
        f = ops.gemm_sigmoid_bce_form(g, q, g2, l)
        assert (f["BN"], f["col_tiles"], f["launches"]) == want
        return
    form = (ctypes.c_int64 * 4)()
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    rc = lib.mst_gemm_sigmoid_bce_form(ref(g), ref(q), ref(g2), ref(l), form)
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg, (rc, msg)
    rc = lib.mst_gemm_sigmoid_bce(ref(g), ref(q), None) if g2 is None else lib.mst_gemm_sigmoid_bce_dgrad_ln(ref(g), ref(q), ref(g2), ref(l), None)
    assert rc == -1 and lib.mst_last_error() == msg


def test_the_engines_own_calls_land_on_forms_the_tables_hold(ops):
    """BASELINE.json's configs[1] (B 64, T 256, 128 pitches) goes through the fused launch with its backward GEMM, as one launch;
    configs[2] (2048 pitches) through mst_gemm_nt + mst_sigmoid_bce: ops.bce_fusion_pays. engine.py passes compact buffers (ld = P)."""
    B, T = 64, 256
    assert ops.can_fuse_bce(128, T) and ops.bce_fusion_pays(128) and ops.ln_bwd_fusion_pays(128)
    c1 = L.FusedCase("configs1", B, T, 128, 128, (128, 1, 1), dgrad=True, drop=0.2)
    f = ops.gemm_sigmoid_bce_form(*_fused_structs(c1, BF))
    assert (f["BN"], f["col_tiles"], f["launches"]) in {c.form for c in L.FUSED_CASES}
    assert ops.can_fuse_bce(2048, T) and not ops.bce_fusion_pays(2048)
    c2 = L.BceCase("configs2", B, T, 2048, 2048, 2048, 2048, (), dw=True)
    f = L.form_tuple(ops.sigmoid_bce_form(**L.bce_form_call(c2, BF)))
    assert f[:4] in {c.form[:4] for c in L.BCE_CASES} and f[4] == 8    # several workgroups per sample, as p128-wide has
    # the decoder's per-position call (decode.py): T = 1, compact rows
    f = L.form_tuple(ops.sigmoid_bce_form(**L.bce_form_call(L.BceCase("dec", 5, 1, 128, 128, 128, 0, (), decoder=True), BF)))
    assert f == L.BCE_CASE["decoder-t1"].form


def test_softmax_cases_reach_the_grid_stride_loop_and_its_edge():
    by = {c.id: c for c in L.CE_CASES}
    assert not L.CeCase("configs1", 64, 256, 10, 16, 16).strided            # 16384 rows: exactly the grid's waves
    assert by["rows16400-stride"].strided and by["rows16405-cross"].strided and not by["v293"].strided
    assert by["rows16400-stride"].M - 16384 > 4                             # a whole workgroup takes a second stride, and more
    # a wave's stride of 16384 rows crosses samples of 3281 rows; 16384 % 3281 != 0
    assert by["rows16405-cross"].T < 16384 and 16384 % by["rows16405-cross"].T
    assert {c.top_k for c in L.CE_CASES} >= {1, 5} and any(c.top_k == c.V for c in L.CE_CASES)
    assert by["v10-pad"].zero_end == 12 and by["v10-ldd10"].zero_end == 10 and by["v293"].zero_end == 296


# ------------------------------------------------------------------------------------------ operands
@pytest.mark.parametrize("run", [r for r in BCE_RUNS + FUSED_RUNS], ids=_id)
def test_operand_modes_are_what_they_say(run):
    c, dtype, mode = run
    x, labels = _bce_xy(c, dtype, mode) if isinstance(c, L.BceCase) else _fused_xy(c, dtype, mode)
    out = ~L.in_domain(x)
    if mode == "real":
        assert np.abs(x).max() <= 8.0 and not out.any()
    elif mode == "known":
        assert not x.any()
    else:
        assert out.mean() >= 0.25
        assert (x <= -25.0).any() and (x >= 17.5).any(), "both sides, beyond the points where the branches differ visibly"
        per_row = out.reshape(-1, c.P).sum(1)
        assert (per_row == 0).any() and (per_row == 1).any() and (per_row == c.P).any(), "rows inside, with one element outside, outside"
        if c.T >= 16:  # ... arranged so that 8 consecutive rows (more than any wave covers) are of one kind
            g = per_row.reshape(c.B, c.T // 8, 8)
            assert (g.sum(2) == 0).any() and (g.sum(2) == 1).any() and (g == c.P).all(2).any()


@pytest.mark.parametrize("run", BCE_RUNS + FUSED_RUNS, ids=_id)
def test_wide_elements_stay_below_one_percent(run):
    c, dtype, mode = run
    x, labels = _bce_xy(c, dtype, mode) if isinstance(c, L.BceCase) else _fused_xy(c, dtype, mode)
    r = L.bce_ref(x, labels, c.ls, c.dw, c.gscale, dtype)
    for name in ("probs", "dlogits"):
        frac = L.is_wide(r[name], r["b_" + name], dtype).mean()
        assert frac <= L.WIDE_CAP, f"{name}: {frac:.4f} of the elements have a bound above four times their rounding"
    if mode == "sat" and c.dw and isinstance(c, L.BceCase) and c.T >= 16:
        assert L.is_wide(r["dlogits"], r["b_dlogits"], dtype).any(), "the planted 13 / 15 are wide: the condition is exercised"


@pytest.mark.parametrize("run", CE_RUNS, ids=_id)
def test_ce_wide_elements_stay_below_one_percent(run):
    c, dtype, mode = run
    r = L.ce_references(c.id, dtype, mode)
    frac = L.is_wide(r["dlogits"], r["b_dlogits"], dtype).mean()
    assert frac <= L.WIDE_CAP, f"{frac:.4f}"
    if mode == "wide":
        lab = L.ce_operands(c.id, dtype, mode)["labels"].numpy()
        pl = r["probs"][np.arange(c.M), lab][lab != 0]
        assert c.decoder or len(pl) == 0 or (pl < 1e-45).any(), "a label's probability underflows"
        assert (r["probs"] < 2.0 ** -149).any()


# ------------------------------------------------------------------------------------------ the bounds accept an honest evaluation
def _inside(got, ref, bound):
    return bool((np.abs(got - ref) <= bound).all())


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("run", BCE_RUNS + FUSED_RUNS, ids=_id)
def test_bce_bounds_accept_an_fp32_emulation(run, order):
    c, dtype, mode = run
    x, labels = _bce_xy(c, dtype, mode) if isinstance(c, L.BceCase) else _fused_xy(c, dtype, mode)
    r = L.bce_ref(x, labels, c.ls, c.dw, c.gscale, dtype)
    e = L.bce_emulate(x, labels, c.ls, c.dw, c.gscale, dtype, order)
    for name in ("probs", "dlogits", "loss"):
        ratio = np.abs(e[name] - r[name]) / np.maximum(r["b_" + name], 1e-300)
        assert ratio.max() <= 1.0, f"{name}: worst error / bound {ratio.max():.3f}"
    assert np.array_equal(e["npos"], r["npos"])
    if mode == "known":
        p, dl, exact = L.bce_known(labels, c.ls, c.dw, c.gscale, c.T, c.P, dtype)
        assert np.array_equal(e["probs"], p) and np.array_equal(e["dlogits"][exact], dl[exact]) and (p == 0.5).all()
        assert _inside(dl, r["dlogits"], r["b_dlogits"])
        if c.ls == 0 and not c.dw:
            assert np.abs(r["loss"] - np.log(2.0)).max() < 1e-11 and np.abs(dl).max() == 0.5 / (c.T * c.P) * c.gscale


def test_known_mode_is_exact_in_fp32_too():
    y = np.array([0, 1], dtype=np.float32)
    for ls in (0.0, 0.1):
        p, bce, d = L.fast32(np.zeros(2, dtype=np.float32), y, ls, np.float32(0), False)
        s = L._s32(y, ls)
        assert (p == 0.5).all() and np.array_equal(d, np.float32(0.5) - s)
        assert ls != 0 or np.array_equal(bce, np.full(2, np.float32(0.6931471805599453)))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("run", CE_RUNS, ids=_id)
def test_ce_bounds_accept_an_fp32_emulation(run, order):
    c, dtype, mode = run
    o = L.ce_operands(c.id, dtype, mode)
    x, labels = o["logits"][:, :c.V].double().numpy(), o["labels"].numpy().astype(np.int64)
    r = L.ce_references(c.id, dtype, mode)
    e = L.ce_ref(x, labels, c, dtype, emulate=order)
    for name in ("probs", "dlogits", "loss"):
        ratio = np.abs(e[name] - r[name]) / np.maximum(r["b_" + name], 1e-300)
        assert ratio.max() <= 1.0, f"{name}: worst error / bound {ratio.max():.3f}"
    assert abs(e["tok"][0] - r["tok"][0]) <= r["b_nll"] and np.array_equal(e["tok"][1:], r["tok"][1:])
    if mode == "known":
        p, dl = L.ce_known(c, labels, dtype)
        assert np.array_equal(e["probs"], p) and _inside(dl, r["dlogits"], r["b_dlogits"]) and _inside(p, r["probs"], r["b_probs"])
        nv = (labels != 0).reshape(c.B, c.T).sum(1)
        assert np.allclose(r["loss"], np.log(c.V) * nv / c.T, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------ ... and refuse a wrong kernel
@pytest.mark.parametrize("mistake", L.BCE_MISTAKES)
def test_bce_bounds_refuse_a_wrong_kernel(mistake):
    """on every case, type and mode where the mistake changes anything, some output the launch produces leaves its bound"""
    applied = 0
    for c, dtype, mode in BCE_RUNS + FUSED_RUNS:
        x, labels = _bce_xy(c, dtype, mode) if isinstance(c, L.BceCase) else _fused_xy(c, dtype, mode)
        want_dl = not getattr(c, "decoder", False) and getattr(c, "with_c", True)
        want_p = getattr(c, "with_probs", True)
        if not L.bce_mistake_applies(mistake, x, labels, c.ls, c.dw, c.gscale, want_dl):
            continue
        if mistake in ("fast_everywhere", "true_1_minus_p"):
            assert mode == "sat"
        e = L.bce_emulate(x, labels, c.ls, c.dw, c.gscale, dtype, 0, mistake)
        e0 = L.bce_emulate(x, labels, c.ls, c.dw, c.gscale, dtype, 0)
        names = ["loss"] + (["probs"] if want_p else []) + (["dlogits"] if want_dl else [])
        if all(np.array_equal(e[n], e0[n]) for n in names):   # (e.g. the neighbour's label at logit 0 without smoothing, forward only)
            continue
        r = L.bce_ref(x, labels, c.ls, c.dw, c.gscale, dtype)
        caught = [n for n in names if not _inside(e[n], r[n], r["b_" + n])]
        assert caught, f"{mistake} passes on {c.id} {L.DT_NAME[dtype]} {mode}"
        applied += 1
    assert applied >= 8, applied


@pytest.mark.parametrize("mistake", L.CE_MISTAKES)
def test_ce_bounds_refuse_a_wrong_kernel(mistake):
    applied = 0
    for c, dtype, mode in CE_RUNS:
        o = L.ce_operands(c.id, dtype, mode)
        x, labels = o["logits"][:, :c.V].double().numpy(), o["labels"].numpy().astype(np.int64)
        if not L.ce_mistake_applies(mistake, x, labels, c):
            continue
        applied += 1
        if mistake == "pad_not_zeroed":   # the check the GPU test makes on the pad columns: zero, not the sentinel
            pad = np.full((c.M, c.zero_end - c.V), L.SENTINEL)
            assert (pad != 0).any()
            continue
        r = L.ce_references(c.id, dtype, mode)
        e = L.ce_ref(x, labels, c, dtype, mistake=mistake, emulate=0)
        caught = not np.array_equal(e["tok"][1:], r["tok"][1:]) or not _inside(e["loss"], r["loss"], r["b_loss"])
        caught = caught or (c.with_dl and not _inside(e["dlogits"], r["dlogits"], r["b_dlogits"]))
        assert caught, f"{mistake} passes on {c.id} {L.DT_NAME[dtype]} {mode}"
    assert applied >= 4, applied


# ------------------------------------------------------------------------------------------ the losses on probabilities
@pytest.mark.parametrize("dtype", L.PROB_DTYPES, ids=lambda d: L.DT_NAME[d])
def test_losses_on_probabilities_references_and_bounds(dtype):
    from vae_oracle import binary_cross_entropy, softmax_cross_entropy
    o = L.probs_operands(dtype)
    B, T, V, n = L.PROBS_B, L.PROBS_T, L.PROBS_V, L.PROBS_N
    p = o["ce_probs"][:, :V].double().numpy()
    lab = o["ce_labels"].numpy().astype(np.int64)
    loss, bound = L.ce_probs_ref(p, lab, B, T)
    want = softmax_cross_entropy(torch.tensor(p).view(B, T, V), torch.tensor(lab).view(B, T))
    assert np.allclose(loss, want.numpy(), rtol=1e-13, atol=0)
    p32 = p.astype(np.float32)
    t32 = np.where(lab != 0, -np.log(p32[np.arange(B * T), lab]), np.float32(0)).astype(np.float32).reshape(B, T)
    for emu in (t32.sum(1, dtype=np.float32) / np.float32(T), np.cumsum(t32[:, ::-1], axis=1, dtype=np.float32)[:, -1] / np.float32(T)):
        assert (np.abs(emu - loss) <= bound).all()
    assert not (np.abs(loss * T / np.maximum((lab != 0).reshape(B, T).sum(1), 1) - loss) <= bound).any(), "the mean over valid tokens is refused"
    bp, bl = o["bce_probs"].double().numpy(), o["bce_labels"].numpy()
    assert (bp == 0).any() and (bp == 1).any()
    for ls in (0.0, 0.1):
        for dw in (False, True):
            loss, bound = L.bce_probs_ref(bp, bl, ls, dw)
            want = binary_cross_entropy(torch.tensor(bp), torch.tensor(bl), from_sigmoid=True, label_smoothing=float(np.float32(ls)),
                                        negative_label_downweighting=dw)
            assert np.allclose(loss, want.numpy(), rtol=1e-12, atol=0)
            w32 = binary_cross_entropy(torch.tensor(bp, dtype=torch.float32), torch.tensor(bl), from_sigmoid=True, label_smoothing=ls,
                                       negative_label_downweighting=dw)
            assert (np.abs(w32.double().numpy() - loss) <= bound).all(), (ls, dw)
            assert (bound <= 2e-4 * np.abs(loss)).all()
            if ls:
                wrong, _ = L.bce_probs_ref(bp, bl, 0.0, dw)
                assert not (np.abs(wrong - loss) <= bound).any()
