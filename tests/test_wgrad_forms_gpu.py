"""Every launch form of mst_gemm_wgrad_batch_flush on a real MI355X against the fp64 reference of tests/wgrad_refs.py: the four tile
forms, the narrow and the uint8-A bodies, interleaved and fallback main loops, plain and guarded loads, carried and divided row
remaps, per-problem M splits, and fp32 atomics against the two-pass scratch reduction with and without the bias rows — bf16 and
fp16, once on integers (exact, no tolerance) and once on reals (every element inside the derived bound)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_refs as W  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(o, case, host, gpu, riders):
    """one flush of the whole batch into fresh outputs -> ([(dW buffer, db buffer)] on the host in fp64, rider results)"""
    probs, bufs = [], []
    for p, h in zip(case.probs, host):
        A, B = h["A"].to(gpu), h["B"].to(gpu)
        dW = torch.full((p.N + 2, p.ldw), W.SENTINEL, dtype=torch.float32, device=gpu)  # two rows behind row N - 1, four columns behind K
        db = torch.full((p.N + 3,), W.SENTINEL, dtype=torch.float32, device=gpu)
        dW[:p.N, :p.K] = torch.from_numpy(h["dW0"]).float().to(gpu)
        db[:p.N] = torch.from_numpy(h["db0"]).float().to(gpu)
        probs.append(o.wgrad_problem(A, B, dW[:p.N, :p.K], db if p.db else None, M=p.M, N=p.N, K=p.K, scale=p.scale,
                                     a_remap=p.remap(p.ta), b_remap=p.remap(p.tb)))
        bufs.append((A, B, dW, db))
    # a scratch buffer full of NaN: a slot the reduction pass reads without its slab having written it shows in the result
    scratch = torch.full((case.scratch_bytes // 4,), float("nan"), device=gpu) if case.scratch_bytes else None
    sums = outers = rd = None
    if riders:
        r = {k: v.to(gpu) for k, v in W.rider_operands(case.dtype).items()}
        rd = dict(sums=[torch.ones(length, device=gpu) for _, _, length in W.SUM_SPECS],
                  outers=[torch.zeros(24, 40, device=gpu), torch.ones(16, 40, device=gpu), torch.ones(16, device=gpu)])
        sums = [o.partial_sum_job(r["part"], n, d, col_off=off, length=length) for (n, off, length), d in zip(W.SUM_SPECS, rd["sums"])]
        outers = [o.outer_job(r["L0"], r["R0"], rd["outers"][0]), o.outer_job(r["L1"], r["R1"][:, :40], rd["outers"][1], rd["outers"][2])]
    assert o.gemm_wgrad_plan(probs, case.scratch_bytes) == W.plan_dict(case.plan), "the launch takes another plan than the case is meant for"
    o.gemm_wgrad_batch(probs, scratch=scratch, sums=sums, outers=outers)
    torch.cuda.synchronize()
    got = [(dW.cpu().double().numpy(), db.cpu().double().numpy()) for _, _, dW, db in bufs]
    return got, (None if rd is None else [t.cpu().double().numpy() for t in rd["sums"] + rd["outers"]])


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_wgrad_batch_form_against_fp64(gpu, case, mode):
    from musicstyletransfer_amd import ops as o
    host, refs = W.operands(case.form, case.dtype, mode), W.references(case.form, case.dtype, mode)
    got, riders = _launch(o, case, host, gpu, case.riders)
    worst = 0.0
    for i, (p, r, (dW, db)) in enumerate(zip(case.probs, refs, got)):
        what = f"{case.id} {mode}: problem {i} ({p.kind}, M={p.M} N={p.N} K={p.K}, split {case.plan.splits[i]})"
        assert np.isfinite(dW).all() and np.isfinite(db).all(), f"{what}: a NaN pad column, skipped row or unwritten scratch slot was read"
        for name, g, ref, S in (("dW", dW[:p.N, :p.K], r["dW"], r["SW"]), ("db", db[:p.N], r["db"], r["Sb"])):
            if mode == "int":
                bad = g != ref
                bound = np.zeros_like(ref)
            else:
                bound = W.wgrad_bound(p.M, ref, S)
                bad = ~(np.abs(g - ref) <= bound)
                worst = max(worst, float(np.max(np.abs(g - ref) / np.maximum(bound, 1e-300))))
            if bad.any():
                g2, ref2, bad2, bound2 = (np.atleast_2d(x.T).T if x.ndim == 1 else x for x in (g, ref, bad, bound))
                err = np.abs(g2 - ref2)
                n, k = np.unravel_index(np.argmax(np.where(bad2, err / np.maximum(bound2, 1e-300), 0)), err.shape)
                rows, cols = np.nonzero(bad2)
                pytest.fail(f"{what}: {int(bad.sum())}/{bad.size} elements of {name} outside the bound; worst at n {n}, k {k}: got {g2[n, k]!r}, "
                            f"want {ref2[n, k]!r}, bound {bound2[n, k]:.3g}; n {rows.min()}..{rows.max()}, k {cols.min()}..{cols.max()}, "
                            f"{len(np.unique(rows))} rows, {len(np.unique(cols))} columns")
        assert (dW[p.N:] == W.SENTINEL).all() and (dW[:, p.K:] == W.SENTINEL).all(), f"{what}: a store outside dW (rows behind N or columns behind K)"
        assert (db[p.N:] == W.SENTINEL).all(), f"{what}: a store behind db[N - 1]"
    if mode == "real":
        print(f"\n{case.id}: plan {W.plan_dict(case.plan)}: worst error / bound {worst:.4f}")
    if case.riders:
        sums, outers = W.rider_refs(W.rider_operands(case.dtype))
        for j, (g, ref) in enumerate(zip(riders, sums + outers)):
            assert np.array_equal(g, ref), f"{case.id} {mode}: rider job {j}"
    if mode == "real" and case.plan.two_pass:
        again, _ = _launch(o, case, host, gpu, False)
        for i, ((dW, db), (dW2, db2)) in enumerate(zip(got, again)):
            assert np.array_equal(dW, dW2), f"{case.id}: problem {i}: the two-pass reduction must be run-to-run deterministic"
            # (two_pass == 1: the bias goes by fp32 atomics, and several slabs adding into one element need not repeat bit for bit:
            # there only the one-slab problems must)
            if case.plan.two_pass == 3 or case.plan.splits[i] == 1:
                assert np.array_equal(db, db2), f"{case.id}: problem {i}: the bias sums must be run-to-run deterministic"
