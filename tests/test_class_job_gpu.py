"""The decoder class table's gradient as a job of the weight-gradient flush (mst_gemm_wgrad_batch_flush_cls) on a real MI355X
against the launch it replaces (class_table_grad_kernel: mst_class_table_grad, and mst_latent_bwd_vec given a table), bit for bit:
riding on the reduction pass beside real weight-gradient problems, column-sum jobs and outer-product jobs, and in the fallback
without a scratch buffer; accumulating into a non-zero table with a leading dimension wider than the row; twice in a row. The launch
itself is held to tests/latent_refs.py's fp64 reference and bound.

Shapes: B 1, 3, 4 (fewer rows than, or exactly one per, batch quarter), 17 (one whole 16-row chunk in no quarter, ragged quarters), 64
(one whole chunk per quarter: the step's) and 65 (a chunk plus a row); Dd 64, 128, 256 (one, two, four whole workgroups) and 100 (a
ragged second workgroup); 1, 2 and 4 classes (one pass of CT_CLS) and 5 (a second pass)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

BS = (1, 3, 4, 17, 64, 65)
DDS = (64, 100, 128, 256)
NCLS = (1, 2, 4, 5)
PAD = 8  # ld_cls = Dd + PAD
SENT = 777.0


def ops():
    from musicstyletransfer_amd import ops as o
    return o


def _operands(B, Dd, ncls, dev):
    rng = np.random.default_rng(1000 * B + 10 * Dd + ncls)
    classes = rng.integers(0, ncls, B).astype(np.int32)
    classes[-1] = ncls - 1  # (the kernel takes the class count from the batch)
    t = rng.standard_normal((B, Dd)).astype(np.float32)
    dcls0 = rng.standard_normal((ncls, Dd)).astype(np.float32)
    tvec = torch.full((B * Dd + 64,), float("nan"), device=dev)  # (NaN behind the rows: nothing past B * Dd is read)
    tvec[: B * Dd] = torch.from_numpy(t).to(dev).view(-1)
    buf = torch.full((ncls, Dd + PAD), SENT, device=dev)
    buf[:, :Dd] = torch.from_numpy(dcls0).to(dev)
    return classes, t, dcls0, torch.from_numpy(classes).to(dev), tvec, buf


@pytest.fixture(scope="module")
def flush(gpu):
    """one weight-gradient batch of the whole-step tile form (1.57 M outputs: 256 x 256 tiles, two-pass with a scratch buffer), a column
    sum and an outer product to ride with it, and what they give WITHOUT a class-table job — computed once, never written again"""
    o = ops()
    g = torch.Generator().manual_seed(5)
    M, N, K = 128, 1536, 1024
    A = (torch.randn(M, N, generator=g) * 0.5).to(torch.bfloat16).to(gpu)
    Bm = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).to(gpu)
    parts = torch.randn(40, 512, generator=g).to(gpu)
    L, Rr = torch.randn(9, 24, generator=g).to(gpu), torch.randn(9, 40, generator=g).to(gpu)
    ws = torch.zeros(2 * 1024 * 1024, device=gpu)

    def outs():
        return dict(dW=torch.zeros(N, K, device=gpu), db=torch.zeros(N, device=gpu), col=torch.ones(512, device=gpu),
                    outer=torch.ones(24, 40, device=gpu), obias=torch.ones(24, device=gpu))

    def run(x, scratch, cls):
        o.gemm_wgrad_batch([o.wgrad_problem(A, Bm, x["dW"], x["db"])], scratch=scratch, sums=[o.partial_sum_job(parts, 40, x["col"])],
                           outers=[o.outer_job(L, Rr, x["outer"], x["obias"])], cls=cls)

    plan = o.gemm_wgrad_plan([o.wgrad_problem(A, Bm, torch.zeros(N, K, device=gpu))], ws.numel() * 4)
    assert plan["form"] == 3 and plan["two_pass"] == 3, plan
    assert o.gemm_wgrad_plan([o.wgrad_problem(A, Bm, torch.zeros(N, K, device=gpu))], 0)["two_pass"] == 0
    want = {}
    for mode, scratch in (("ride", ws), ("fallback", None)):
        want[mode] = outs()
        run(want[mode], scratch, None)
    torch.cuda.synchronize()
    # (bf16 products are exact in fp32; M + 2 roundings of the sum and the add into dW)
    ref, mag = A.double().t() @ Bm.double(), A.double().abs().t() @ Bm.double().abs()
    for mode in want:
        assert ((want[mode]["dW"].double() - ref).abs() <= (M + 2) * R.U * mag).all(), mode
        assert ((want[mode]["db"].double() - A.double().sum(0)).abs() <= (M + 2) * R.U * A.double().abs().sum(0)).all(), mode
    return dict(run=run, outs=outs, ws=ws, want=want)


@pytest.mark.parametrize("Dd", DDS)
@pytest.mark.parametrize("B", BS)
def test_job_equals_the_launch(gpu, flush, B, Dd):
    o = ops()
    for ncls in NCLS:
        classes_np, t, dcls0, classes, tvec, buf0 = _operands(B, Dd, ncls, gpu)
        # the launch, into a non-zero table
        want = buf0.clone()
        o.class_table_grad(o.class_job(classes, tvec, want[:, :Dd], B, Dd))
        torch.cuda.synchronize()
        got = want[:, :Dd].double().cpu().numpy()
        ref = R.class_table(t.astype(np.float64), classes_np, dcls0.astype(np.float64), np.float64)
        S = R.class_table(np.abs(t).astype(np.float64), classes_np, np.abs(dcls0).astype(np.float64), np.float64)
        n = np.bincount(classes_np, minlength=ncls)[:, None]
        err, bound = np.abs(got - ref), (n + 4) * R.U * S  # (latent_refs.bwd_refs' bound of dcls)
        print(f"B {B} Dd {Dd} classes {ncls}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all(), (B, Dd, ncls)
        assert (want[:, Dd:] == SENT).all() and not (want[:, :Dd] == buf0[:, :Dd]).all()
        # the job: on the reduction pass and behind a flush without one, each twice
        for mode, scratch in (("ride", flush["ws"]), ("fallback", None)):
            for rep in range(2):
                x, tab = flush["outs"](), buf0.clone()
                flush["run"](x, scratch, o.class_job(classes, tvec, tab[:, :Dd], B, Dd))
                torch.cuda.synchronize()
                assert torch.equal(tab, want), (mode, rep, B, Dd, ncls)
                for k, v in flush["want"][mode].items():  # ... and the jobs it rides beside are what they are without it
                    assert torch.equal(x[k], v), (mode, rep, k)


def test_flush_without_problems_runs_the_job_as_a_launch(gpu):
    o = ops()
    _, _, _, classes, tvec, buf0 = _operands(17, 100, 5, gpu)
    want, tab = buf0.clone(), buf0.clone()
    o.class_table_grad(o.class_job(classes, tvec, want[:, :100], 17, 100))
    o.gemm_wgrad_batch([], cls=o.class_job(classes, tvec, tab[:, :100], 17, 100))
    torch.cuda.synchronize()
    assert torch.equal(tab, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_latent_bwd_without_a_table_leaves_the_same_rows(gpu, dtype):
    """mst_latent_bwd_vec with dcls_d NULL + the job == mst_latent_bwd_vec with the table: scratch, d(enc_out) and the table, bit for bit"""
    o = ops()
    B, S, De, Z, Dd, ncls = 17, 3, 72, 16, 100, 5
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(gpu)
    Wl, Wh, eps, mu = rnd(2 * Z, De, scale=0.2), rnd(Dd, Z, scale=0.3), rnd(B, Z), rnd(B, Z)
    sigma = rnd(B, Z).abs() + 0.5
    g0 = rnd(B, S, Dd, scale=0.1).to(dtype)
    classes = torch.randint(0, ncls, (B,), generator=g, dtype=torch.int32)
    classes[-1] = ncls - 1
    classes = classes.to(gpu)
    buf0 = rnd(ncls, Dd + PAD)
    res = []
    for table in (True, False):
        tab, denc = buf0.clone(), torch.zeros(B, S, De, dtype=dtype, device=gpu)
        scratch = torch.zeros(B * (Dd + 2 * Z), device=gpu)
        o.latent_bwd_vec(Wl, eps, Wh, classes, mu, sigma, g0, math.sqrt(Dd), 0.7, 1.0, tab[:, :Dd] if table else None, denc, scratch)
        if not table:
            torch.cuda.synchronize()
            assert torch.equal(tab, buf0)  # nothing touched it
            o.gemm_wgrad_batch([], cls=o.class_job(classes, scratch, tab[:, :Dd], B, Dd))
        torch.cuda.synchronize()
        res.append((tab, denc, scratch))
    for a, b, name in zip(res[0], res[1], ("dcls", "denc", "scratch")):
        assert torch.equal(a, b), name
    assert not torch.equal(res[0][0], buf0)
