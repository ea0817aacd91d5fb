"""mst_gemm_nt without a GPU: the case table of tests/gemm_refs.py reaches every kernel form the launch can take (asked of
mst_gemm_nt_form, the launch's own decision), the keep decision restated there equals csrc/common.hpp's, and the derived tolerance
accepts a correct fp32 evaluation and refuses the wrong results a GEMM epilogue is prone to."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_refs as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _form(lib, c, **over):
    from musicstyletransfer_amd import _lib
    return lib.mst_gemm_nt_form(ctypes.byref(G.form_args(c, _lib.GemmArgs, **over)))


def _case(code, dtype=G.BF, tag=""):
    return next(c for c in G.CASES if c.code == code and c.dtype == dtype and c.tag == tag)


# ------------------------------------------------------------------------------------------ coverage of the forms
def test_abi_103_exports_the_form_query(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 103
    assert len(_lib.SIGNATURES["mst_gemm_nt_form"][1]) == 1


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
def test_the_cases_reach_exactly_the_31_forms(lib, dtype):
    """fails when a dispatch condition moves and the table no longer covers a form"""
    assert len(G.ALL_CODES) == 31
    reached = set()
    for c in G.CASES:
        if c.dtype != dtype:
            continue
        rc = _form(lib, c)
        assert rc == c.code, f"{c.id}: meant for form {c.code}, the launch takes {rc} ({lib.mst_last_error()})"
        reached.add(rc)
    assert reached == set(G.ALL_CODES)


def test_case_ids_are_unique_and_operands_match_the_layout():
    assert len({c.id for c in G.CASES}) == len(G.CASES)
    c = _case(6)
    o, L = G.operands(c), G.layout(c)
    assert o["A"].shape == (L["A_rows"], c.K) and o["resid"].shape == (L["R_rows"], L["ldr"]) and o["gate"].shape == (c.M, L["ldg"])
    assert G.phys_rows(c)[:3].tolist() == [1, 2, 3] and G.phys_rows(c)[c.T] == c.T + 2


@pytest.mark.parametrize("over,code,why", [
    # three per CU: 513..768 tiles, fast form without dropout / row ops; anything else falls through
    (dict(), 48, "57 x 9 = 513 tiles"),
    (dict(M=8192, N=1024, K=64), 32, "512 tiles are not more than 512"),
    (dict(M=10240, N=1024), 48, "640 tiles"),
    (dict(M=10240, N=1024, K=64, dropout_p=0.25), 33, "640 tiles with dropout: two per CU, the dropout kernel"),
    (dict(M=10240, N=1024, K=72), 34, "K % 32 != 0 is not eligible, and K % 64 != 0 is general"),
    (dict(K=64, dropout_p=0.25), 1, "513 tiles fall through to a stub round of one tile: 64 x 64 tiles"),
    (dict(M=7296 + 128 * 29, K=64), 32, "774 tiles are more than 768"),
])
def test_three_per_cu_eligibility_and_its_fall_through(lib, over, code, why):
    assert _form(lib, _case(48), **over) == code, why


@pytest.mark.parametrize("code,over,want,why", [
    (32, dict(M=6016), 0, "47 x 8 = 376 tiles are fewer than 384"),
    (32, dict(M=6144 + 64), 0, "ragged128: whole 64-row tiles, not whole 128-row tiles"),
    (16, dict(K=768), 16, "K = 768 is three 256-deep stages"),
    (16, dict(K=576), 0, "K % 256 != 0"),
    (16, dict(K=256), 0, "K < 512"),
    (16, dict(M=128), 0, "M > 64"),
    (0, dict(self_resid=1), 1, "self_resid alone takes the dropout kernel"),
    (0, dict(ldc=132), 2, "ldc % 8 != 0 is general"),
    (0, dict(resid=4104), 2, "a residual off 16 bytes is general"),
    (4, dict(rowadd_period=96), 6, "a period that is not whole tiles is general"),
])
def test_dispatch_conditions_at_their_edges(lib, code, over, want, why):
    assert _form(lib, _case(code), **over) == want, why


@pytest.mark.parametrize("over,text", [
    (dict(K=12), b"multiples of 8"), (dict(M=0), b"must be positive"), (dict(ldc=126), b"ldc must be"), (dict(A=None), b"null operand"),
    (dict(ldr=64), b"ldr must be"), (dict(ldg=130), b"ldg must be"), (dict(dropout_p=1.0), b"dropout_p must be"),
    (dict(B=4100), b"16-byte aligned"), (dict(a_u8=1, c_f32=1), b"uint8 A operand"),
    (dict(rowadd=4096, rowadd_period=0), b"rowadd_period"), (dict(grpadd=4096, rowadd_period=8), b"grp_index"),
])
def test_the_form_query_rejects_what_the_launch_rejects(lib, over, text):
    """validation comes before any HIP call in both: same status, same message"""
    from musicstyletransfer_amd import _lib
    g = G.form_args(_case(0), _lib.GemmArgs, **over)
    rc = lib.mst_gemm_nt_form(ctypes.byref(g))
    msg = lib.mst_last_error()
    assert rc == -1 and text in msg, (rc, msg)
    assert lib.mst_gemm_nt(ctypes.byref(g), None) == -1 and lib.mst_last_error() == msg
    assert lib.mst_gemm_nt_form(None) == -1 and b"null args" in lib.mst_last_error()
    assert _form(lib, _case(0), dtype=2) == -3 and b"unsupported activation dtype" in lib.mst_last_error()
    g = G.form_args(_case(2, tag="drop"), _lib.GemmArgs, N=70)
    assert lib.mst_gemm_nt_form(ctypes.byref(g)) == -1 and b"dropout needs N" in lib.mst_last_error()


# ------------------------------------------------------------------------------------------ the keep decision
PROBE = r"""
#include <stdio.h>
#include <inttypes.h>
#include "common.hpp"
using namespace mst;
int main() {
  const uint64_t seeds[3] = {0ull, 0x0123456789ABCDEFull, 0xFFFFFFFFFFFFFFFFull};
  const uint32_t sites[3] = {0u, 3u, 0xFFFFFFFFu};
  const uint64_t idx[8] = {0ull, 1ull, 2ull, 3ull, 1000003ull, 0xFFFFFFFFull, 0x200000001ull, 0x123456789ABCull};
  const float ps[3] = {0.1f, 0.2f, 0.5f};
  for (int s = 0; s < 3; ++s)
    for (int t = 0; t < 3; ++t) {
      printf("key %" PRIu32 "\n", dropout_key(seeds[s], sites[t]));
      for (int i = 0; i < 8; ++i) {
        printf("word %" PRIu32 "\n", dropout_word(dropout_key(seeds[s], sites[t]), idx[i] >> 1));
        for (int p = 0; p < 3; ++p) printf("keep %d\n", (int)dropout_keep(seeds[s], sites[t], idx[i], ps[p]));
      }
    }
  for (int p = 0; p < 3; ++p) printf("thr %" PRIu32 " %.9g\n", dropout_thr(ps[p]), (double)dropout_inv_keep(ps[p]));
  // the two restatements the epilogues use agree with dropout_word below 2^32
  const uint32_t key = dropout_key(seeds[1], sites[1]);
  int same = 1;
  for (uint32_t w = 0; w < 4096; ++w) {
    float a[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {1.f, 1.f, 1.f, 1.f}, c[4] = {1.f, 1.f, 1.f, 1.f};
    const uint32_t i4 = w * 524287u + 5u;
    dropout_apply4(key, (uint64_t)i4, dropout_thr(0.2f), 1.25f, a);
    dropout_apply4_32(key, i4, dropout_thr(0.2f), 1.25f, b);
    dropout_apply4_pre(key, (2u * i4) * DROPOUT_MUL, dropout_thr(0.2f), 1.25f, c);
    for (int e = 0; e < 4; ++e) same &= (a[e] == b[e]) & (a[e] == c[e]) & ((a[e] != 0.f) == dropout_keep(seeds[1], sites[1], 4ull * i4 + e, 0.2f));
  }
  printf("same %d\n", same);
  return 0;
}
"""
P_SEEDS = (0, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF)
P_SITES = (0, 3, 0xFFFFFFFF)
P_IDX = (0, 1, 2, 3, 1000003, 0xFFFFFFFF, 0x200000001, 0x123456789ABC)
P_PS = (0.1, 0.2, 0.5)


def test_keep_mask_equals_common_hpp():
    """known answers from a few lines of host C++ that include csrc/common.hpp: the key, the word (also past 2^32, where the high half
    of the index enters), the decision, the threshold and the scale; and the epilogues' restatements (dropout_word32, the
    pre-multiplied form) agree with dropout_word where they are used"""
    from musicstyletransfer_amd.csrc import build
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
        open(src, "w").write(PROBE)
        subprocess.check_call([build.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-I", os.path.join(ROOT, "musicstyletransfer_amd", "csrc"),
                               src, "-o", exe])
        got = iter(subprocess.check_output([exe], text=True).split())

    def nxt(name):
        assert next(got) == name
        return next(got)

    for seed in P_SEEDS:
        for site in P_SITES:
            key = G.dropout_key(seed, site)
            assert key == int(nxt("key"))
            for i in P_IDX:
                assert int(G.dropout_words(key, [i >> 1])[0]) == int(nxt("word")), (seed, site, i)
                for p in P_PS:
                    assert bool(G.keep_mask(seed, site, [i], p)[0][0]) == bool(int(nxt("keep"))), (seed, site, i, p)
    for p in P_PS:
        assert G.dropout_thr(p) == int(nxt("thr"))
        assert abs(G.keep_mask(0, 0, [0], p)[1] - float(next(got))) <= 2.0 ** -23 * 2
    assert nxt("same") == "1"
    assert [G.dropout_thr(p) for p in P_PS] == [6553, 13107, 32768]


@pytest.mark.parametrize("p", P_PS)
def test_keep_fraction_is_the_exact_keep_probability(p):
    n = 1 << 20
    keep, scale = G.keep_mask(G.SEED, G.SITE, np.arange(n, dtype=np.uint64), p)
    q = (65536 - G.dropout_thr(p)) / 65536
    assert abs(keep.mean() - q) <= 4 * math.sqrt(q * (1 - q) / n), (keep.mean(), q)
    assert scale == 1 / q
    # the two fields of a word are not the same decision, and another site is another mask
    assert (keep[0::2] != keep[1::2]).mean() > 0.5 * 2 * q * (1 - q)
    other, _ = G.keep_mask(G.SEED, G.SITE + 1, np.arange(n, dtype=np.uint64), p)
    assert (other != keep).mean() > 0.5 * 2 * q * (1 - q)


# ------------------------------------------------------------------------------------------ the bound discriminates
def torch_eval(c, o, wrong=None):
    """the operation in fp32 torch, rounded to the output type -> fp64 [M, N]; `wrong`: one deliberate mistake"""
    f32 = torch.float32
    pm = torch.from_numpy(G.phys_rows(c))
    m = torch.arange(c.M)
    A, B = o["A"][pm].to(f32), o["B"].to(f32)
    if wrong == "k_dropped":
        A = A.clone()
        A[c.M // 2, c.K // 2] = 0  # one k term of one output row (its operand was not zero: checked by the caller)
    bias = o["bias"].clone()
    if wrong == "bias_moved":
        bias[5] = o["bias"][4]
    t = A @ B.t() + bias
    if c.T:
        t = t + o["grpadd"][o["grp_index"].long()[m // c.T]]
    t = torch.relu(t * torch.tensor(G.ALPHA, dtype=f32))
    if c.p > 0:
        rows = m if wrong == "logical_counter" else pm
        idx = rows.numpy().astype(np.uint64)[:, None] * np.uint64(c.N) + np.arange(c.N, dtype=np.uint64)[None, :]
        keep, scale = G.keep_mask(G.SEED ^ G.SEED_WORD, G.SITE, idx, c.p)
        u = t * torch.from_numpy(keep) * torch.tensor(scale, dtype=f32)
        t = t + u if c.self_resid else u
    elif c.self_resid:
        t = t + t
    if c.T:
        t = t + o["rowadd"][(m + (1 if wrong == "rowadd_shifted" else 0)) % c.T]
    r = o["resid"][pm if (c.T and c.resid_phys) else m, :c.N].to(f32)
    open_ = o["gate"][:, :c.N].to(f32) > 0
    t = torch.where(open_, t, torch.zeros(())) + r if wrong == "gate_first" else torch.where(open_, t + r, torch.zeros(()))
    return (t if c.c_f32 else t.to(c.dtype)).double().numpy()


WRONG = ("k_dropped", "rowadd_shifted", "logical_counter", "bias_moved", "gate_first")


@pytest.mark.parametrize("code", [5, 16 + 5, 32 + 5, 48], ids=lambda c: f"tile{c >> 4}")
def test_the_bound_takes_fp32_and_refuses_wrong_results(code):
    """one case per tile form (the fast row-op dropout variant where the form has one: it has every operand). A correct fp32
    evaluation is inside gemm_bound everywhere; each wrong result is outside it somewhere"""
    c = _case(code)
    o = G.operands(c)
    ref, S = G.gemm_ref(c, o)
    bound = G.gemm_bound(c, ref, S)
    err = np.abs(torch_eval(c, o) - ref)
    assert (err <= bound).all(), f"{c.id}: fp32 evaluation outside the bound at {int((err > bound).sum())} elements, worst ratio {np.max(err / bound):.3g}"
    assert bound.max() < 0.05 * np.abs(ref).max(), "a bound of the size of the result would accept anything"
    assert o["A"][G.phys_rows(c)[c.M // 2], c.K // 2] != 0
    applicable = [w for w in WRONG if (c.T or w != "rowadd_shifted") and (c.p > 0 or w != "logical_counter")]
    assert code == 48 or applicable == list(WRONG)
    for w in applicable:
        bad = np.abs(torch_eval(c, o, wrong=w) - ref) > bound
        assert bad.any(), f"{c.id}: the bound accepts `{w}`"
        if w == "k_dropped":
            assert not np.delete(bad, c.M // 2, axis=0).any(), "one row's mistake must not show elsewhere"
