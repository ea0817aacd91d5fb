"""Every launch form of the latent block on a real MI355X against the staged fp64 references of tests/latent_refs.py: the preloaded
and the general forward with both loaders in both products, the row-0 projection at its three widths, the backward pass preloaded,
four-column and scalar, its read and its computed (proj) form, the class table over one to three passes, and the deferred outer
products — bf16 and fp16, once on integers (the exact quantities compared with ==) and once on reals (every element inside its
derived bound). Outputs sit in sentinel-filled buffers and strided inputs carry NaN pad columns; every launch runs twice and must
repeat bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
S = 2  # positions per sample in the strided buffers: only position 0 belongs to the latent block


def dev(x, dtype, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(gpu)


def rows3(x, pad, dtype, gpu):
    """x [B, n] as position 0 of a [B, S, n + pad] buffer whose other positions and pad columns hold NaN -> the [B, S, n] view"""
    buf = torch.full((x.shape[0], S, x.shape[1] + pad), NAN, dtype=dtype, device=gpu)
    buf[:, 0, :x.shape[1]] = dev(x, dtype, gpu)
    return buf[:, :, :x.shape[1]]


def padded(x, pad, dtype, gpu):
    buf = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=dtype, device=gpu)
    buf[:, :x.shape[1]] = dev(x, dtype, gpu)
    return buf[:, :x.shape[1]]


def out3(B, n, dtype, gpu):
    """-> (buffer [B + 2, S, n + PAD] of sentinels, the [B, S, n] view a launch writes position 0 of)"""
    buf = torch.full((B + 2, S, n + R.PAD), R.SENTINEL, dtype=dtype, device=gpu)
    return buf, buf[:B, :, :n]


def untouched3(buf, B, n):
    """everything but [:B, 0, :n] still holds the sentinel"""
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:B, 0, :n] = False
    return bool((buf[keep] == R.SENTINEL).all())


def flat_out(x0, gpu):
    """an accumulated fp32 output pre-filled with x0, 64 sentinels behind it -> (buffer, contiguous view of x0's shape)"""
    buf = torch.full((x0.size + 64,), R.SENTINEL, dtype=torch.float32, device=gpu)
    buf[:x0.size] = dev(x0, torch.float32, gpu).reshape(-1)
    return buf, buf[:x0.size].view(*x0.shape)


def np64(t):
    return t.detach().double().cpu().numpy()


def report(c, dtype, mode, verdict):
    for k, (bad, ratio, msg) in verdict.items():
        assert not bad, msg
    if mode == "real":
        print(f"\n{c.id} {R.DT_NAME[dtype]}: form {c.form}: worst error / bound " + ", ".join(f"{k} {v[1]:.4f}" for k, v in verdict.items() if k != "t16"))


# ------------------------------------------------------------------------------------------ forward
def launch_fwd(o, c, h, dtype, gpu):
    """one forward launch into fresh sentinel-filled outputs -> (the buffers, what it stored as fp64 arrays)"""
    f = torch.float32
    B, De, Z, Dd = c.B, c.De, c.Z, c.Dd
    enc = rows3(h["h"], R.PAD, dtype, gpu)
    Wl, bl, eps = dev(h["Wl"], f, gpu), dev(h["bl"], f, gpu), dev(h["eps"], f, gpu)
    Wh, bh = dev(h["Wh"], f, gpu), dev(h["bh"], f, gpu)
    cls = padded(h["cls"], 3, f, gpu)
    pos = torch.full((3, Dd), NAN, device=gpu)
    pos[0] = dev(h["pos"], f, gpu)
    classes = dev(h["classes"], torch.int32, gpu)
    bufs = {k: torch.full((B + 2, Z), R.SENTINEL, device=gpu) for k in ("mu", "sigma", "z")}
    bufs["kl"] = torch.full((B + 2,), R.SENTINEL, device=gpu)
    bufs["dec"], dec = out3(B, Dd, dtype, gpu)
    proj = None
    if c.nq:
        bufs["qkv"] = torch.full((B + 2, S, c.nq + c.qkv_pad), R.SENTINEL, dtype=dtype, device=gpu)
        proj = (padded(h["Wq"], c.wq_pad, dtype, gpu), dev(h["bq"], f, gpu) if c.bq else None, bufs["qkv"][:B, :, :c.nq])
    assert o.latent_form(De, Z, Dd, c.nq, Wl, part="fwd") == dict(zip(("fwd_pre", "loader_l", "loader_h", "proj_vec", "fwd_lds"), c.form))
    o.latent_fwd(enc, Wl, bl, eps, Wh, bh, classes, cls, pos, h["alpha"], bufs["mu"], bufs["sigma"], bufs["z"], bufs["kl"], dec, proj=proj)
    torch.cuda.synchronize()
    got = {k: np64(bufs[k][:B]) for k in ("mu", "sigma", "z", "kl")}
    got["dec"] = np64(bufs["dec"][:B, 0, :Dd])
    if c.nq:
        got["qkv"] = np64(bufs["qkv"][:B, 0, :c.nq])
    return bufs, got


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("c", R.FWD, ids=lambda c: c.id)
def test_latent_fwd_form_against_fp64(gpu, c, dtype, mode):
    from musicstyletransfer_amd import ops as o
    h = R.operands(c, dtype, mode)
    bufs, got = launch_fwd(o, c, h, dtype, gpu)
    what = f"{c.id} {R.DT_NAME[dtype]} {mode}"
    for k in ("mu", "sigma", "z", "kl"):
        assert (bufs[k][c.B:] == R.SENTINEL).all(), f"{what}: a store behind {k}"
    assert untouched3(bufs["dec"], c.B, c.Dd), f"{what}: dec_in written outside position 0 (rows >= 1, pad columns or samples behind B)"
    assert not c.nq or untouched3(bufs["qkv"], c.B, c.nq), f"{what}: qkv written outside position 0"
    assert all(np.isfinite(v).all() for v in got.values()), f"{what}: a NaN pad column or row was read"
    report(c, dtype, mode, R.judge(c, h, dtype, mode, got))
    again, _ = launch_fwd(o, c, h, dtype, gpu)
    for k in bufs:
        assert torch.equal(bufs[k], again[k]), f"{what}: {k} differs between two runs"


# ------------------------------------------------------------------------------------------ backward
def launch_bwd(o, c, h, dtype, gpu, sched=False):
    f = torch.float32
    B, De, Z, Dd = c.B, c.De, c.Z, c.Dd
    wl = torch.zeros(2 * Z * De + 4, device=gpu)
    Wl = wl[c.wl_off:c.wl_off + 2 * Z * De].view(2 * Z, De)
    Wl.copy_(dev(h["Wl"], f, gpu))
    assert Wl.data_ptr() % 16 == 4 * c.wl_off
    Wh, eps, mu, sigma = (dev(h[k], f, gpu) for k in ("Wh", "eps", "mu", "sigma"))
    classes = dev(h["classes"], torch.int32, gpu)
    bufs = dict(dcls=torch.full((c.ncls + 2, Dd + 3), R.SENTINEL, device=gpu),
                scratch=torch.full(((B + 2) * (Dd + 2 * Z),), R.SENTINEL, device=gpu))
    bufs["dcls"][:c.ncls, :Dd] = dev(h["dcls0"], f, gpu)
    bufs["denc"], denc = out3(B, De, dtype, gpu)
    proj = None
    if c.nq:
        g3 = rows3(h["dq"], R.PAD, dtype, gpu)
        proj = (g3, padded(h["Wt"], c.wt_pad, dtype, gpu), rows3(h["resid"], R.PAD, dtype, gpu) if c.resid else None)
    else:
        g3 = rows3(h["g"], R.PAD, dtype, gpu)
    assert o.latent_form(De, Z, Dd, c.nq, Wl, part="bwd") == dict(zip(("bwd_pre", "dh0", "bwd_lds"), c.form))
    klw, gscale, enc_scale = h["klw"], h["gscale"], h["enc_scale"]
    sc = (torch.tensor([klw, 0.5, 0.0, 0.0], device=gpu), torch.ones(B, device=gpu)) if sched else None  # (every kl above the allowance)
    o.latent_bwd_vec(Wl, eps, Wh, classes, mu, sigma, g3, h["alpha"], klw, gscale, bufs["dcls"][:c.ncls, :Dd], denc, bufs["scratch"],
                     enc_scale=enc_scale, proj=proj, sched=sc)
    # the deferred parameter gradients, from the scratch rows as stored
    outs = [flat_out(x0, gpu) for x0 in h["out0"]]
    enc, z = rows3(h["h"], R.PAD, dtype, gpu), dev(h["z"], f, gpu)
    o.outer_jobs(o.latent_outer_jobs(bufs["scratch"], enc, z, *(v for _, v in outs)))
    torch.cuda.synchronize()
    for k, (buf, _) in zip(("dWl", "dbl", "dWh", "dbh"), outs):
        bufs[k] = buf
    got = dict(t=np64(bufs["scratch"][:B * Dd].view(B, Dd)), dlat=np64(bufs["scratch"][B * Dd:B * (Dd + 2 * Z)].view(B, 2 * Z)),
               denc=np64(bufs["denc"][:B, 0, :De]), dcls=np64(bufs["dcls"][:c.ncls, :Dd]))
    got.update({k: np64(v) for k, (_, v) in zip(("dWl", "dbl", "dWh", "dbh"), outs)})
    return bufs, got


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("c", R.BWD, ids=lambda c: c.id)
def test_latent_bwd_form_against_fp64(gpu, c, dtype, mode):
    from musicstyletransfer_amd import ops as o
    h = R.operands(c, dtype, mode)
    bufs, got = launch_bwd(o, c, h, dtype, gpu)
    what = f"{c.id} {R.DT_NAME[dtype]} {mode}"
    n = c.B * (c.Dd + 2 * c.Z)
    assert (bufs["scratch"][n:] == R.SENTINEL).all(), f"{what}: a store behind the scratch rows"
    assert (bufs["dcls"][c.ncls:] == R.SENTINEL).all() and (bufs["dcls"][:, c.Dd:] == R.SENTINEL).all(), f"{what}: a store outside the class table"
    assert untouched3(bufs["denc"], c.B, c.De), f"{what}: d_enc_out written outside position 0"
    for k in ("dWl", "dbl", "dWh", "dbh"):
        assert (bufs[k][-64:] == R.SENTINEL).all(), f"{what}: a store behind {k}"
    assert all(np.isfinite(v).all() for v in got.values()), f"{what}: a NaN pad column or row was read"
    report(c, dtype, mode, R.judge(c, h, dtype, mode, got))
    # twice the same bytes (the class table too: the kernel is handed no table, its atomic branch is dead), and the scheduled
    # launch at kl_weight = beta with every sample above the allowance
    for name, sched in (("two runs", False),) + ((("the scheduled launch", True),) if c.sched and not c.nq else ()):
        again, _ = launch_bwd(o, c, h, dtype, gpu, sched=sched)
        for k in bufs:
            assert torch.equal(bufs[k], again[k]), f"{what}: {k} differs between {name}"


# ------------------------------------------------------------------------------------------ outer products on their own
def outer_launch(o, launch, host, gpu, how):
    """the jobs of one launch into fresh pre-filled outputs: as a launch of their own, or as riders of a weight-gradient flush with
    (scratch) / without (flush) a reduction pass -> the output buffers"""
    jobs, bufs, alive = [], [], []  # (a job holds addresses, not tensors: its operands must outlive the launch)
    for q, h in zip(launch, host):
        L = dev(h["L"], torch.float32, gpu)
        Rm = padded(h["R"], q.r_pad, R.R_DTYPE[q.r], gpu)
        ob, out = flat_out(h["out0"], gpu)
        bb, bias = flat_out(h["bias0"], gpu) if q.bias else (None, None)
        jobs.append(o.outer_job(L, Rm, out, bias))
        alive += [L, Rm]
        bufs += [ob] + ([bb] if q.bias else [])
    if how == "own":
        o.outer_jobs(jobs)
    else:
        g = torch.Generator().manual_seed(5)
        # one problem of the 256 x 256 tile form, the only one with a reduction pass: 1536 x 1024 outputs, 24 tiles in two slabs
        A, Bm = torch.randn((256, 1536), generator=g).to(R.BF).to(gpu), torch.randn((256, 1024), generator=g).to(R.BF).to(gpu)
        ws = torch.zeros(4 << 20, device=gpu) if how == "scratch" else None
        prob = [o.wgrad_problem(A, Bm, torch.zeros(1536, 1024, device=gpu))]
        assert o.gemm_wgrad_plan(prob, 16 << 20 if ws is not None else 0)["two_pass"] == (3 if how == "scratch" else 0)
        o.gemm_wgrad_batch(prob, scratch=ws, outers=jobs)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("i", range(len(R.OUTER)))
def test_outer_jobs_against_fp64(gpu, i, mode):
    from musicstyletransfer_amd import ops as o
    launch, host = R.OUTER[i], R.outer_operands(mode)[i]
    bufs = outer_launch(o, launch, host, gpu, "own")
    it, worst = iter(bufs), 0.0
    for q, h in zip(launch, host):
        (ref, bound), bias = R.outer_refs(h["L"], h["R"], h["out0"], h["bias0"])
        for name, rb in (("out", (ref, bound)),) + ((("obias", bias),) if q.bias else ()):
            buf = next(it)
            g = np64(buf[:rb[0].size]).reshape(rb[0].shape)
            assert (buf[rb[0].size:] == R.SENTINEL).all(), f"{q} {mode}: a store behind {name}"
            if mode == "int":
                assert np.array_equal(g, rb[0]), f"{q}: {name}"
            else:
                assert (np.abs(g - rb[0]) <= rb[1]).all(), f"{q}: {name}: worst error / bound {np.max(np.abs(g - rb[0]) / rb[1]):.3f}"
                worst = max(worst, float(np.max(np.abs(g - rb[0]) / rb[1])))
    if mode == "real":
        print(f"\nouter launch {i}: worst error / bound {worst:.4f}")
    hows = ("own",) + (("scratch", "flush") if i == len(R.OUTER) - 1 else ())  # the ragged 70-row launch also rides on a flush
    for how in hows:
        for a, b in zip(bufs, outer_launch(o, launch, host, gpu, how)):
            assert torch.equal(a, b), f"outer launch {i} ({mode}): {how} differs from the launch of its own"
