"""All 18 instantiations of csrc/attention_causal.hip on a real MI355X against the fp64 reference of tests/causal_refs.py: forward,
query-owner and key-owner backward at head sizes 16, 32 and 64, bf16 and fp16 — one row to nine blocks, every kind of key mask
(rows without keys included), contiguous, widened and permuted layouts, on unit-scale operands and on operands whose running maximum
arrives in the last block (`late`) or in the first with everything later underflowing (`early`). Every element inside the derived
bound, every byte outside the results untouched, every launch bit-identical when repeated."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import causal_refs as C  # noqa: E402

pytestmark = pytest.mark.gpu
_failed = []   # the case whose launch raised (a HIP error): the cases after it fail without touching the GPU


def _check(what, r, got, name):
    """every element of got[name] inside its bound (lse on a row without keys: -inf itself); -> worst error / bound. Failures as
    test_attn_forms_gpu._check reports them"""
    g, ref, bound = got[name], r[name], np.broadcast_to(r["b_" + name], got[name].shape)
    bad, ratio = C.violations(r, got, name), C.ratios(r, got, name)
    if bad.any():
        g2, r2, b2, bad2, ratio2 = (x.reshape(-1, x.shape[-1]) for x in (g, ref, bound, bad, ratio))
        i, j = np.unravel_index(np.argmax(np.where(bad2, np.maximum(np.nan_to_num(ratio2, nan=np.inf), 1e-300), 0)), bad2.shape)
        rows, cols = np.nonzero(bad2)
        pytest.fail(f"{what}: {int(bad.sum())}/{bad.size} elements of {name} outside the bound; worst at row {i}, column {j} of "
                    f"{g2.shape}: got {g2[i, j]!r}, want {r2[i, j]!r}, bound {b2[i, j]:.3g}; rows {rows.min()}..{rows.max()}, columns "
                    f"{cols.min()}..{cols.max()}, {len(np.unique(rows))} rows, {len(np.unique(cols))} columns")
    return float(ratio.max())


def _run(o, c, dev, dtype, gpu):
    """forward and backward into fresh sentinel-filled buffers, two rows (lse, delta: two words) longer than the results; the
    backward reads the lse the forward wrote, as the training step does"""
    B, S, H, dh = c.B, c.S, c.H, c.dh
    ldq, ldo, lddo = c.lds
    full = lambda rows, ld, dt=dtype: torch.full((rows, ld), C.SENTINEL, dtype=dt, device=gpu)  # noqa: E731
    out, dqkv = full(B * S + 2, ldo), full(B * S + 2, ldq)
    lse, delta = full(1, 2 * B * H * S + 2, torch.float32)[0], full(1, B * H * S + 2, torch.float32)[0]
    lse2 = lse[:2 * B * H * S].view(2, B, H, S)
    o.attn_causal_fwd(dev["qkv"], dev["keymask"], lse2, out[:B * S], B, S, H, dh, *c.offs)
    o.attn_causal_bwd(dev["qkv"], dev["keymask"], lse2, dev["dout"], dqkv[:B * S], delta[:B * H * S].view(B, H, S), B, S, H, dh, *c.offs)
    torch.cuda.synchronize()
    return dict(out=out, dqkv=dqkv, lse=lse, delta=delta)


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: C.DT_NAME[d])
@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c.id)
def test_causal_attention_against_fp64(gpu, c, dtype, mode):
    from musicstyletransfer_amd import ops as o
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    what = f"{c.id} {C.DT_NAME[dtype]} {mode}"
    host = C.operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    assert not _failed, f"an earlier launch failed ({_failed[0]}): nothing more is launched"
    try:
        first = _run(o, c, dev, dtype, gpu)
        again = _run(o, c, dev, dtype, gpu)
    except Exception:
        _failed.append(what)
        raise
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), again[k].view(torch.uint8)), f"{what}: {k} differs between two launches: there are no atomics"
    g = {k: v.cpu().double().numpy() for k, v in first.items()}
    r = C.references(c.id, dtype, mode)

    # every store is where it belongs: behind the last row, in every pad column, behind lse and delta the sentinels stand
    out, dqkv, lse, delta = g["out"], g["dqkv"], g["lse"], g["delta"]
    assert (out[B * S:] == C.SENTINEL).all() and (out[:, D:] == C.SENTINEL).all(), f"{what}: a store behind the last row of out or into its pad columns"
    assert (dqkv[B * S:] == C.SENTINEL).all() and (dqkv[:, 3 * D:] == C.SENTINEL).all(), f"{what}: a store behind the last row of dqkv or into its pad columns"
    assert (lse[2 * B * H * S:] == C.SENTINEL).all(), f"{what}: a store behind lse"
    assert (delta[B * H * S:] == C.SENTINEL).all(), f"{what}: a store behind delta"

    lse2 = lse[:2 * B * H * S].reshape(2, B, H, S)
    got = dict(out=out[:B * S, :D].reshape(B, S, H, dh), lse=lse2[0] + lse2[1], delta=delta[:B * H * S].reshape(B, H, S))
    for name, off in zip(("dK", "dQ", "dV"), c.offs):
        got[name] = dqkv[:B * S, off:off + D].reshape(B, S, H, dh)
    # the rows without keys: lse0 (and lse1) exactly -inf, out exactly 0; everything else finite — no NaN pad column was read
    empty = ~np.isfinite(r["lse0"])                                    # [B, H, S]
    assert (lse2[0][empty] == -np.inf).all() and (lse2[1][empty] == -np.inf).all(), f"{what}: lse on a row without keys is not -inf"
    assert not got["out"].transpose(0, 2, 1, 3)[empty].any(), f"{what}: out on a row without keys is not 0"
    assert np.isfinite(lse2[:, ~empty]).all(), f"{what}: lse holds a non-finite value on a row with keys"
    for name in ("out", "delta", "dQ", "dK", "dV"):
        assert np.isfinite(got[name]).all(), f"{what}: {name} holds a non-finite value (a NaN pad column or an unwritten element was read)"

    worst = {name: _check(what, r, got, name) for name in C.RESULTS}
    print(f"\n{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
