"""attention_causal.hip on a real GPU: the causal key-softmax attention forward (O and the per-query statistics) and backward
(dQ | dK | dV, delta) against fp32 torch autograd on the same 16-bit Q / K / V, plus the properties the training step relies on:
later rows and padded rows do not reach earlier outputs, identical calls give identical bits, graph replay equals eager."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 2


def _case(gpu, B, S, dh, dtype, ragged, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + S * 31 + dh)
    D = H * dh
    qkv = (torch.randn(B * S, 3 * D, generator=g) * 1.5).to(dtype).to(gpu)
    dout = torch.randn(B * S, D, generator=g).to(dtype).to(gpu)
    lens = torch.full((B,), S - 1, dtype=torch.int64)
    if ragged:
        lens = torch.randint(0, S, (B,), generator=g)
        lens[0] = S - 1
    keymask = (torch.arange(S)[None, :] < (lens[:, None] + 1)).to(torch.uint8).to(gpu)  # the decoder's mask: k < len + 1
    return qkv, dout, keymask


def _bufs(gpu, B, S, dh, dtype):
    D = H * dh
    return dict(lse=torch.full((2, B, H, S), float("nan"), device=gpu), out=torch.zeros(B * S, D, dtype=dtype, device=gpu),
                dqkv=torch.zeros(B * S, 3 * D, dtype=dtype, device=gpu), delta=torch.zeros(B, H, S, device=gpu))


def _run(o, qkv, dout, keymask, bf, B, S, dh):
    D = H * dh
    o.attn_causal_fwd(qkv, keymask, bf["lse"], bf["out"], B, S, H, dh, 0, D, 2 * D)
    o.attn_causal_bwd(qkv, keymask, bf["lse"], dout, bf["dqkv"], bf["delta"], B, S, H, dh, 0, D, 2 * D)


def _reference(qkv, dout, keymask, B, S, dh):
    D = H * dh
    x = qkv.float().cpu().view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)  # [3, B, H, S, dh]
    K, Q, V = x[0], x[1], x[2]
    logits = Q @ K.transpose(-1, -2) / math.sqrt(dh)
    allowed = torch.ones(S, S, dtype=torch.bool).tril()[None, None] & (keymask.cpu() > 0)[:, None, None, :]
    logits = logits.masked_fill(~allowed, float("-inf"))
    probs = torch.softmax(logits, -1)
    out = probs @ V  # [B, H, S, dh]
    go = dout.float().cpu().view(B, S, H, dh).transpose(1, 2)
    out.backward(go)
    rmax = logits.max(-1).values
    logl = torch.log(torch.exp(logits - rmax[..., None]).sum(-1))
    delta = (go * out).sum(-1)
    dqkv = x.grad.permute(1, 3, 0, 2, 4).reshape(B * S, 3 * D)
    return out.detach().transpose(1, 2).reshape(B * S, D), torch.stack([rmax, logl]).detach(), dqkv, delta.detach()


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("S", [1, 2, 31, 32, 33, 64, 65, 257, 1025])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_causal_attention_matches_fp32_autograd(gpu, dh, S, ragged, dtype):
    from musicstyletransfer_amd import ops as o
    B = 3 if S <= 257 else 2
    qkv, dout, keymask = _case(gpu, B, S, dh, dtype, ragged)
    bf = _bufs(gpu, B, S, dh, dtype)
    _run(o, qkv, dout, keymask, bf, B, S, dh)
    torch.cuda.synchronize()
    out, stats, dqkv, delta = _reference(qkv, dout, keymask, B, S, dh)
    tol = 1.2e-2 if dtype == torch.bfloat16 else 3e-3  # (P and dS enter their products as 16-bit operands)
    assert _rel(bf["out"], out) <= tol
    assert torch.allclose(bf["lse"].cpu(), stats, rtol=1e-4, atol=1e-4)
    assert torch.allclose(bf["delta"].cpu(), delta, rtol=2 * tol, atol=2 * tol * float(delta.abs().max()))
    D = H * dh
    for nm, sl in (("dK", slice(0, D)), ("dQ", slice(D, 2 * D)), ("dV", slice(2 * D, 3 * D))):
        want = dqkv[:, sl]
        if float(want.norm()) == 0.0:  # (S 1: one key, P = 1 and dK = dQ = 0 up to the rounding of dP - delta)
            assert float(bf["dqkv"][:, sl].float().abs().max()) <= 1e-5 * float(dqkv.abs().max()), nm
            continue
        assert _rel(bf["dqkv"][:, sl], want) <= 2 * tol, nm


@pytest.mark.parametrize("dh", [16, 32, 64])
def test_future_rows_and_padding_do_not_reach_earlier_outputs(gpu, dh):
    from musicstyletransfer_amd import ops as o
    B, S, dtype = 3, 97, torch.bfloat16
    D = H * dh
    qkv, dout, keymask = _case(gpu, B, S, dh, dtype, ragged=True, seed=3)
    lens = keymask.sum(1).cpu() - 1
    a = _bufs(gpu, B, S, dh, dtype)
    _run(o, qkv, dout, keymask, a, B, S, dh)
    # forward: rewrite Q | K | V rows after q, and put large finite garbage into every padded key's K | V rows
    q = 40
    qkv2 = qkv.clone().view(B, S, 3 * D)
    qkv2[:, q + 1:] = torch.randn_like(qkv2[:, q + 1:].float()).to(dtype) * 3
    for b in range(B):
        qkv2[b, int(lens[b]) + 1:, :D] = 3.0e4 if dtype == torch.float16 else 1e30
        qkv2[b, int(lens[b]) + 1:, 2 * D:] = -3.0e4 if dtype == torch.float16 else -1e30
    qkv2 = qkv2.view(B * S, 3 * D)
    b_ = _bufs(gpu, B, S, dh, dtype)
    o.attn_causal_fwd(qkv2, keymask, b_["lse"], b_["out"], B, S, H, dh, 0, D, 2 * D)
    torch.cuda.synchronize()
    for b in range(B):
        n = q + 1  # rows 0..q (padded query rows included) attend to unchanged, valid keys only
        rows = slice(b * S, b * S + n)
        assert torch.equal(a["out"][rows], b_["out"][rows]), b
        assert torch.equal(a["lse"][:, b, :, :n], b_["lse"][:, b, :, :n]), b


def test_identical_calls_are_bit_identical_and_graph_replay_equals_eager(gpu):
    from musicstyletransfer_amd import ops as o
    B, S, dh, dtype = 8, 257, 16, torch.bfloat16
    qkv, dout, keymask = _case(gpu, B, S, dh, dtype, ragged=True, seed=5)
    runs = []
    for _ in range(2):
        bf = _bufs(gpu, B, S, dh, dtype)
        _run(o, qkv, dout, keymask, bf, B, S, dh)
        torch.cuda.synchronize()
        runs.append({k: v.clone() for k, v in bf.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    bf = _bufs(gpu, B, S, dh, dtype)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g = o.Graph().capture(lambda: _run(o, qkv, dout, keymask, bf, B, S, dh))
        g.launch()
    torch.cuda.synchronize()
    for k in runs[0]:
        assert torch.equal(bf[k], runs[0][k]), k
