"""The W_proj input gradient inside the attention-backward launch (ops.attn_proj_bwd) on a real MI355X: bit for bit against the two
launches it replaces (ops.gemm_nt into datt, then ops.attn_bwd), and against the fp64 reference of tests/attn_refs.py — the dO the
launch stores against dproj Wt^T with the bound of a product rounded once (attn_refs.qkv_ref), then dK, dQ, dV and delta of THAT dO
with the reference's own bounds. Shapes outside the fused form run the two launches inside the call. One host-only test pins which
shapes take the projection inside the launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_refs as A  # noqa: E402

BF, FP = A.BF, A.FP


def _case(B, S, H, dh, masks):
    return A.Case(id=f"proj_{B}x{S}x{H}x{dh}", B=B, S=S, H=H, dh=dh, fwd="", bwd="", masks=masks)


# (case, dtype, projection inside the launch, dproj / Wt / dO row strides beyond D)
CASES = (
    (_case(2, 256, 8, 32, ("full", "mid")), BF, 1, (0, 0, 0)),       # the encoder layer of the step: whole tiles
    (_case(3, 200, 4, 32, ("full", "mid", "tile")), BF, 1, (0, 0, 0)),  # ragged: padded-key tiles, a partial last row block
    (_case(5, 96, 2, 32, ("full", "mid")), FP, 1, (0, 0, 0)),        # D = 64: a single slice
    (_case(2, 257, 8, 16, ("full", "mid")), BF, 1, (0, 0, 0)),       # the decoder of the step: the lone row, SP 288
    (_case(3, 33, 4, 16, ("full", "mid")), FP, 1, (0, 0, 0)),        # one full block plus the lone row; D = 64
    (_case(2, 64, 2, 32, ("full", "mid")), BF, 1, (8, 16, 8)),       # strided operands, NaN in their pad columns
    (_case(1, 1024, 2, 32, ("full",)), BF, 0, (0, 0, 0)),            # streaming backward: the GEMM launch first
    (_case(1, 100, 1, 64, ("mid",)), BF, 0, (0, 0, 0)),              # head size 64: the GEMM launch first
)


def _operands(c, dtype, pads):
    """deterministic operands of a case: qkv [B S, 3 D], keymask, dproj [B S, D + pad] ~ N(0, 1), Wt [D, D + pad] ~ N(0, 1 / D); pad
    columns NaN. The decoder shape keeps the position-0 rows of dproj at zero, as the step leaves them"""
    rng = np.random.default_rng([c.B, c.S, c.H, c.dh, A.DTYPES.index(dtype), 20262])
    B, S, D = c.B, c.S, c.D
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dtype)  # noqa: E731

    def padded(a, pad):
        full = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=dtype)
        full[:, :a.shape[1]] = t(a)
        return full

    dproj = rng.standard_normal((B, S, D))
    if c.dh == 16:
        dproj[:, 0] = 0.0
    return dict(qkv=t(rng.standard_normal((B * S, 3 * D))), keymask=torch.from_numpy(c.valid().astype(np.uint8)),
                dproj=padded(dproj.reshape(B * S, D), pads[0]), Wt=padded(rng.standard_normal((D, D)) / np.sqrt(D), pads[1]))


def _sentinel(gpu, c, dtype, pad):
    B, S, H, D = c.B, c.S, c.H, c.D
    full = lambda rows, ld, dt=dtype: torch.full((rows, ld), A.SENTINEL, dtype=dt, device=gpu)  # noqa: E731
    return dict(dout=full(B * S + 2, D + pad), dqkv=full(B * S + 2, 3 * D), delta=full(1, B * H * S + 2, torch.float32)[0])


def _args(c, dev, lse, r):
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    return (dev["qkv"], dev["keymask"], lse), (r["dqkv"][:B * S], r["delta"][:B * H * S].view(B, H, S), B, S, H, dh, 0, D, 2 * D)


def _bytes_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _within(what, name, got, ref, bound):
    assert np.isfinite(got).all(), f"{what}: {name} holds a non-finite value (a pad column or an unwritten element was read)"
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    assert (np.abs(got - ref) <= bound).all(), f"{what}: {name} outside the bound, worst error / bound {ratio.max():.3f}"
    return float(ratio.max())


@pytest.mark.gpu
@pytest.mark.parametrize("c, dtype, inside, pads", CASES, ids=[f"{c.id}-{A.DT_NAME[d]}" for c, d, _, _ in CASES])
def test_projection_inside_the_backward_launch_equals_gemm_then_attention(gpu, monkeypatch, c, dtype, inside, pads):
    from musicstyletransfer_amd import ops as o
    monkeypatch.delenv("MST_ATTN_PATH", raising=False)
    B, S, H, dh, D = c.B, c.S, c.H, c.dh, c.D
    what = f"{c.id} {A.DT_NAME[dtype]}"
    form = o.attn_bwd_form(dtype, B, S, H, dh, 0, D, 2 * D, 3 * D, D + pads[2], 3 * D, proj=True)
    assert form["proj"] == inside, "the call takes another plan than the case is meant for"
    host = _operands(c, dtype, pads)
    dev = {k: v.to(gpu) for k, v in host.items()}
    dproj, Wt = dev["dproj"][:, :D], dev["Wt"][:, :D]
    lse = torch.zeros(2, B, H, S, dtype=torch.float32, device=gpu)
    o.attn_fwd(dev["qkv"], dev["keymask"], lse, torch.empty(B * S, D, dtype=dtype, device=gpu), B, S, H, dh, 0, D, 2 * D)

    # the two launches
    two = _sentinel(gpu, c, dtype, pads[2])
    head, tail = _args(c, dev, lse, two)
    datt = two["dout"][:B * S, :D]
    o.gemm_nt(dproj, Wt, datt, N=D, K=D)
    o.attn_bwd(*head, datt, *tail)
    # the one call, storing dO; again (two launches of it agree); without the store
    runs = []
    for store in (True, True, False):
        r = _sentinel(gpu, c, dtype, pads[2])
        head, tail = _args(c, dev, lse, r)
        if store or inside:
            o.attn_proj_bwd(*head, dproj, Wt, *tail, dout_out=r["dout"][:B * S, :D] if store else None)
        else:  # the GEMM launch has to write dO somewhere: refused before anything is launched
            with pytest.raises(RuntimeError, match="needs dout_out"):
                o.attn_proj_bwd(*head, dproj, Wt, *tail)
            r = dict(two, dout=r["dout"])
        runs.append(r)
    torch.cuda.synchronize()
    one, again, bare = runs
    for k in ("dout", "dqkv", "delta"):
        assert _bytes_equal(one[k], again[k]), f"{what}: {k} differs between two launches: there are no atomics"
        assert _bytes_equal(one[k], two[k]), f"{what}: {k} is not the two launches' bit for bit (sentinel rows and columns included)"
    assert _bytes_equal(bare["dqkv"], two["dqkv"]) and _bytes_equal(bare["delta"], two["delta"]), f"{what}: results differ without dout_out"
    assert (bare["dout"] == A.SENTINEL).all(), f"{what}: dO was stored although dout_out is null"
    g = {k: v.cpu() for k, v in one.items()}
    assert (g["dout"][B * S:] == A.SENTINEL).all() and (g["dout"][:, D:] == A.SENTINEL).all(), f"{what}: a store outside dO"
    assert (g["dqkv"][B * S:] == A.SENTINEL).all() and (g["delta"][B * H * S:] == A.SENTINEL).all(), f"{what}: a store behind dqkv or delta"

    # fp64: the product rounded once, then the attention backward of the dO the launch stored
    ref, bound = A.qkv_ref(c, dict(x=host["dproj"], W=host["Wt"], bias=torch.zeros(D)), dtype)
    dO = g["dout"][:B * S, :D]
    worst = dict(dO=_within(what, "dO", dO.double().numpy(), ref, bound))
    r = A.reference_on(c, host["qkv"], dO, dtype)
    dqkv = g["dqkv"].double().numpy()
    for name, off in zip(("dK", "dQ", "dV"), c.offs):
        worst[name] = _within(what, name, dqkv[:B * S, off:off + D].reshape(B, S, H, dh), r[name], r["b_" + name])
    worst["delta"] = _within(what, "delta", g["delta"].double().numpy()[:B * H * S].reshape(B, H, S), r["delta"], r["b_delta"])
    print(f"\n{what}: backward {form['path']} {form['waves']} waves, projection {'inside' if inside else 'as a GEMM launch'}; "
          "worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_the_form_query_reports_where_the_projection_runs():
    """inside the launch for the two shapes of the step, in both activation types; as the GEMM launch for the sparse kernel (the top
    encoder layer), the streaming paths and head size 64. Host only: no launch, no device."""
    from musicstyletransfer_amd import ops as o
    os.environ.pop("MST_ATTN_PATH", None)
    q = lambda dt, B, S, H, dh, ql=0: o.attn_bwd_form(dt, B, S, H, dh, 0, H * dh, 2 * H * dh, 3 * H * dh, H * dh, 3 * H * dh, ql, proj=True)  # noqa: E731
    for dt in (BF, FP):
        enc, dec = q(dt, 64, 256, 8, 32), q(dt, 64, 257, 8, 16)
        assert enc["proj"] == 1 and enc["path"] == "resident" and enc["waves"] == 8
        assert dec["proj"] == 1 and dec["path"] == "resident" and dec["waves"] == 8 and dec["lone"] == 1
        assert q(dt, 64, 256, 8, 32, ql=1)["proj"] == 0 and q(dt, 64, 256, 8, 32, ql=1)["sparse"] == 1
        assert q(dt, 16, 1024, 8, 32)["proj"] == 0 and q(dt, 16, 1024, 8, 32)["path"] != "resident"
        assert q(dt, 16, 1025, 8, 16)["proj"] == 0
        assert q(dt, 64, 256, 4, 64)["proj"] == 0 and q(dt, 64, 256, 4, 64)["path"] == "resident"
    # without the keyword the query returns what it always did
    assert "proj" not in o.attn_bwd_form(BF, 64, 256, 8, 32, 0, 256, 512, 768, 256, 768)
