"""Every launch form of mst_gemm_nt on a real MI355X against the fp64 reference of tests/gemm_refs.py: each of the 31 kernel forms
(tile shape x stage depth x epilogue variant), bf16 and fp16, with every operand the variant admits, every logical element inside
the derived bound, the pad columns exact zeros and the rest of C's buffer untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_refs as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_gemm_nt_form_against_fp64(gpu, case):
    from musicstyletransfer_amd import ops as o
    c, L = case, G.layout(case)
    host = G.operands(c)
    dev = {k: v.to(gpu) for k, v in host.items()}
    C = torch.full((L["C_rows"], c.ldc), G.SENTINEL, dtype=torch.float32 if c.c_f32 else c.dtype, device=gpu)
    kw = G.call_kwargs(c, dev)
    assert o.gemm_nt_form(dev["A"], dev["B"], C, **kw) == c.code, "the launch takes another form than the case is meant for"
    o.gemm_nt(dev["A"], dev["B"], C, **kw)
    torch.cuda.synchronize()
    got = C.cpu().double().numpy()
    ref, S = G.gemm_ref(c, host)
    bound = G.gemm_bound(c, ref, S)
    pm = G.phys_rows(c)
    err = np.abs(got[pm, :c.N] - ref)
    bad = ~(err <= bound)
    if bad.any():
        r, n = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
        rows, cols = np.nonzero(bad)
        pytest.fail(f"{c.id}: {int(bad.sum())}/{bad.size} elements outside the bound; worst at row {r} (physical {pm[r]}), column {n}: "
                    f"got {got[pm[r], n]!r}, want {ref[r, n]!r}, bound {bound[r, n]:.3g}; rows {rows.min()}..{rows.max()}, "
                    f"columns {cols.min()}..{cols.max()}, {len(np.unique(rows))} rows, {len(np.unique(cols))} columns")
    n4 = min(G.roundup(c.N, 4), c.ldc)
    assert (got[pm, c.N:n4] == 0).all(), "columns N..min(roundup4(N), ldc) must be exact zeros"
    untouched = np.ones(got.shape, dtype=bool)
    untouched[pm, :n4] = False
    assert untouched.any() == (c.ldc > n4 or c.T > 0)
    assert (got[untouched] == G.SENTINEL).all(), "a store outside the output: columns beyond roundup4(N) or a row outside the C remap"


def test_dropout_mask_kernel_equals_keep_mask(gpu):
    """the library's own mask (what the older GEMM tests compare with) against the restated decision, element by element"""
    from musicstyletransfer_amd import ops as o
    n = 100003  # not a multiple of 4
    for seed in (G.SEED, 1):
        for site in (0, G.SITE):
            for p in (0.2, 0.5):
                keep = torch.full((n + 5,), 9, dtype=torch.uint8, device=gpu)
                o.dropout_mask(n, p, seed, site, keep)
                torch.cuda.synchronize()
                want, _ = G.keep_mask(seed, site, np.arange(n, dtype=np.uint64), p)
                k = keep.cpu().numpy()
                assert np.array_equal(k[:n], want.astype(np.uint8)), (seed, site, p)
                assert (k[n:] == 9).all(), "the mask kernel wrote past n"
