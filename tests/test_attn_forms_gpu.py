"""Every launch form of key-row attention on a real MI355X against the fp64 reference of tests/attn_refs.py: the forward on three
tiles, on two, chunked, with the projection fused in, and streaming; the backward resident, streaming with dQ in one or two chunks
and with the streaming dQ; dense and sparse, with and without the lone row, every kind of key mask, q_limit from 1 to beyond S,
padded and permuted layouts — bf16 and fp16, on unit-scale reals and on `big` integers (padded rows that are not uniform). Every
element inside the derived bound, every byte outside the results untouched, every launch bit-identical when repeated."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_refs as A  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(what, name, got, ref, bound, exact=False):
    """every element of got within bound of ref (exact: equal); -> worst error / bound. Failures as the wgrad suite reports them"""
    assert np.isfinite(got).all(), f"{what}: {name} holds a non-finite value (a NaN pad column or an unwritten element was read)"
    err = np.abs(got - ref)
    bad = (got != ref) if exact else ~(err <= bound)
    ratio = err / np.maximum(bound, 1e-300)
    if bad.any():
        g2, r2, b2, bad2, ratio2 = (x.reshape(-1, x.shape[-1]) for x in (got, ref, np.broadcast_to(bound, got.shape), bad, ratio))
        i, j = np.unravel_index(np.argmax(np.where(bad2, np.maximum(ratio2, 1e-300), 0)), bad2.shape)
        rows, cols = np.nonzero(bad2)
        pytest.fail(f"{what}: {int(bad.sum())}/{bad.size} elements of {name} outside the bound; worst at row {i}, column {j} of "
                    f"{g2.shape}: got {g2[i, j]!r}, want {r2[i, j]!r}, bound {b2[i, j]:.3g}; rows {rows.min()}..{rows.max()}, columns "
                    f"{cols.min()}..{cols.max()}, {len(np.unique(rows))} rows, {len(np.unique(cols))} columns")
    return 0.0 if exact else float(ratio.max())


def _run(o, c, dev, dtype, gpu):
    """forward (or the fused call) and backward into fresh sentinel-filled buffers, two rows longer than the results"""
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    ldq, ldo, lddo, ldx, ldw = c.lds
    full = lambda rows, ld, dt=dtype: torch.full((rows, ld), A.SENTINEL, dtype=dt, device=gpu)  # noqa: E731
    out, dqkv = full(B * S + 2, ldo), full(B * S + 2, ldq)
    lse, delta = full(1, 2 * B * H * S + 2, torch.float32)[0], full(1, B * H * S + 2, torch.float32)[0]
    lse2 = lse[:2 * B * H * S].view(2, B, H, S)
    if c.fused:
        qkv = full(B * S + 2, ldq)
        o.attn_qkv_fwd(dev["x"][:, :D], dev["W"][:, :D], dev["bias"], qkv[:B * S], dev["keymask"], lse2, out[:B * S], B, S, H, dh, *c.offs,
                       q_limit=c.q_limit)
    else:
        qkv = dev["qkv"]
        o.attn_fwd(qkv, dev["keymask"], lse2, out[:B * S], B, S, H, dh, *c.offs, q_limit=c.q_limit)
    o.attn_bwd(qkv[:B * S], dev["keymask"], lse2, dev["dout"], dqkv[:B * S], delta[:B * H * S].view(B, H, S), B, S, H, dh, *c.offs,
               q_limit=c.q_limit)
    torch.cuda.synchronize()
    return dict(out=out, dqkv=dqkv, lse=lse, delta=delta, qkv=qkv)


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("dtype", A.DTYPES, ids=lambda d: A.DT_NAME[d])
@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.id)
def test_attention_form_against_fp64(gpu, monkeypatch, c, dtype, mode):
    from musicstyletransfer_amd import ops as o
    if c.force:
        monkeypatch.setenv("MST_ATTN_PATH", c.force)
    else:
        monkeypatch.delenv("MST_ATTN_PATH", raising=False)
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    ldq, ldo, lddo, ldx, ldw = c.lds
    what = f"{c.id} {A.DT_NAME[dtype]} {mode}"
    fa, ba = A.form_calls(c, dtype)
    f, b = o.attn_fwd_form(*fa), o.attn_bwd_form(*ba)
    assert not A.check_forms(c, f, b), "the launch takes another plan than the case is meant for"

    host = A.operands(c.id, dtype, mode)
    dev = {k: v.to(gpu) for k, v in host.items()}
    got = _run(o, c, dev, dtype, gpu)
    again = _run(o, c, dev, dtype, gpu)
    for k in ("out", "dqkv", "lse", "delta") + (("qkv",) if c.fused else ()):
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), f"{what}: {k} differs between two launches: there are no atomics"
    g = {k: v.cpu() for k, v in got.items()}

    worst = {}
    if c.fused:  # the projection itself, then the attention of the qkv the launch wrote (what the backward pass reads)
        ref, bound = A.qkv_ref(c, host, dtype)
        qkv = g["qkv"]
        worst["qkv"] = _check(what, "qkv", qkv[:B * S, :3 * D].double().numpy(), ref, bound, exact=(mode == "big"))
        assert (qkv[B * S:] == A.SENTINEL).all() and (qkv[:, 3 * D:] == A.SENTINEL).all(), f"{what}: a store outside qkv"
        r = A.reference_on(c, qkv[:B * S], host["dout"], dtype, mode)
    else:
        r = A.references(c.id, dtype, mode)
    ql = c.q_limit if 0 < c.q_limit < S else S
    valid = c.valid(mode)

    out = g["out"].double().numpy()
    out4 = out[:B * S, :D].reshape(B, S, H, dh)
    worst["out"] = _check(what, "out", out4[:, :ql], r["out"][:, :ql], r["b_out"][:, :ql])
    assert (out4[:, ql:] == A.SENTINEL).all(), f"{what}: a row of out at or beyond q_limit was written"
    assert (out[B * S:] == A.SENTINEL).all() and (out[:, D:] == A.SENTINEL).all(), f"{what}: a store behind the last row of out or into its pad columns"

    lse = g["lse"].double().numpy()
    lse2 = lse[:2 * B * H * S].reshape(2, B, H, S)
    worst["lse"] = _check(what, "lse[0] + lse[1]", lse2[0] + lse2[1], r["lse"], r["b_lse"])
    pad = np.broadcast_to(~valid[:, None, :], (B, H, S))
    if pad.any():  # a padded row's maximum is an fp32 number near -1e9, the reference's bit for bit (in `big` mode not -1e9 itself)
        _check(what, "lse[0] on the padded rows", lse2[0][pad][None], r["lse0"][pad][None], 0.0, exact=True)
    assert (lse[2 * B * H * S:] == A.SENTINEL).all(), f"{what}: a store behind lse"

    dqkv = g["dqkv"].double().numpy()
    for name, off in zip(("dK", "dQ", "dV"), c.offs):
        worst[name] = _check(what, name, dqkv[:B * S, off:off + D].reshape(B, S, H, dh), r[name], r["b_" + name])
    assert (dqkv[B * S:] == A.SENTINEL).all() and (dqkv[:, 3 * D:] == A.SENTINEL).all(), f"{what}: a store behind the last row of dqkv or into its pad columns"
    delta = g["delta"].double().numpy()
    worst["delta"] = _check(what, "delta", delta[:B * H * S].reshape(B, H, S), r["delta"], r["b_delta"])
    assert (delta[B * H * S:] == A.SENTINEL).all(), f"{what}: a store behind delta"
    print(f"\n{what}: forward {f['path']} {f['waves']} waves, backward {b['path']} {b['waves']} waves; worst error / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
