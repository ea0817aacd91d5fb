"""The one-launch position-0 tails on a real MI355X against the fp64 reference of tests/tail_refs.py: mst_row_tail_fwd, _fwd_ride,
_fwd_ride_shadows, mst_row_tail_bwd and _bwd_ride in all six kernel instantiations per direction, bf16 and fp16, on hard operands in
a layout whose every row stride differs, every stored tensor held stage by stage to its derived bound, every pad column, guard row
and row that is not a position-0 row left alone; the riding GEMM bit-identical to mst_gemm_nt and inside its fp64 bound, the
shadows exact transposes; two launches give the same bits; and, for four cases, a second launch with other operands into the same
buffers gives its own result, not a stale row of the first. A launch that comes up short (barrier counter, status word, tile
queue) fails before any number is looked at; nothing is retried."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_refs as T  # noqa: E402

pytestmark = pytest.mark.gpu


def _view(c, bufs, t, name):
    """the [B, width] row view the launch takes (stride(0): the buffer's row stride in elements), or the weight without its pad"""
    b = bufs[name]
    if b.rows == "phys":
        return t[:c.M * b.stride:b.stride, :b.width]
    return t[:, :b.width] if b.rows == "w" else t


def _rider_kw(r, C_out):
    K, N, Tt = r["K"], r["N"], r["T"]
    kw = dict(A=r["A"][:, :K], B=r["W"][:, :K], C_out=C_out[:r["A"].shape[0], :N], M=r["M"], N=N, K=K, a_remap=(Tt, Tt + 1, 1),
              c_remap=(Tt, Tt + 1, 1))
    if "bias" in r:
        kw["bias"] = r["bias"]
    else:
        kw.update(resid=r["resid"][:, :N], resid_phys=True)
    return kw


class Launch:
    """one direction of a case on the device: its rider, its shadows, its sync / status / queue words"""

    def __init__(self, o, c, backward, gpu, with_rider=True):
        self.o, self.c, self.backward, self.gpu = o, c, backward, gpu
        self.form = dict(T.case_forms(c))[backward] if with_rider else T.ride_form(backward, c.D)
        self.rider = self.shadows = None
        if with_rider and c.rider != "none":
            self.rider = {k: (v.to(gpu) if isinstance(v, torch.Tensor) else v) for k, v in T.rider_operands(c, backward).items()}
            if c.shadows and not backward:
                self.sh_host = T.shadow_operands(c)
                self.shadows = {k: (v.to(gpu) if isinstance(v, torch.Tensor) else v) for k, v in self.sh_host.items()}

    def run(self, i, u):
        """launch into u (inputs: i, and for a chain's backward half the forward's outputs in u); the launch must have done all of
        its work before anything is compared"""
        o, c, D = self.o, self.c, self.c.D
        bufs, _ = T.plan(c)
        v = lambda n: _view(c, bufs, u[n] if bufs[n].out else i[n], n)  # noqa: E731
        sync = torch.zeros(8, dtype=torch.int32, device=self.gpu)
        status = torch.zeros(4, dtype=torch.int32, device=self.gpu)
        queue = torch.zeros(64, dtype=torch.int32, device=self.gpu)[32:33]
        kw = dict(stat_stride=T.STAT_STRIDE, phys_stride=T.PHYS_STRIDE, dropout_p=c.p, dropout_seed=T.SEED, dropout_seed_ptr=i["seed_word"],
                  site0=T.SITE0, status=status[0:1])
        if self.rider is not None:
            self.C = self.rider["C"].clone()
            kw.update(rider=_rider_kw(self.rider, self.C), queue=queue)
            got = o.row_tail_form(self.backward, c.dtype, D, kw["rider"], self.shadows["tiles"] if self.shadows else 0)
        else:
            got = o.row_tail_form(self.backward, c.dtype, D)
        assert got == self.form, f"{c.id}: mst_row_tail_form {got} against the restatement {self.form}"
        if self.backward:
            o.row_tail_bwd(v("dy"), v("h2"), v("h1"), v("a"), v("mean1"), v("rstd1"), v("mean2"), v("rstd2"), v("g1"), v("g2"), v("W2t"), v("W1t"),
                           v("Wpt"), v("dh"), v("dhm"), v("dx1"), v("dh1m"), v("dpre"), v("dh1"), v("datt"), u["dg1"], u["db1"], u["dg2"], u["db2"],
                           sync[0:3], **kw)
        else:
            if self.shadows is not None:
                self.wt16 = self.shadows["wt16"].clone()
                kw["shadows"] = dict(w=self.shadows["w"], wt16=self.wt16, desc=self.shadows["desc"], prefix=self.shadows["prefix"],
                                     n_mat=self.shadows["n_mat"], tiles=self.shadows["tiles"])
            o.row_tail_fwd(v("att"), v("resid"), v("Wp"), v("bp"), v("g1"), v("be1"), v("W1"), v("b1"), v("W2"), v("b2"), v("g2"), v("be2"),
                           v("h1"), v("x1"), v("a"), v("h2"), v("x2"), v("mean1"), v("rstd1"), v("mean2"), v("rstd2"), sync[0:3], **kw)
        torch.cuda.synchronize()
        which = "backward" if self.backward else "forward"
        want = o.row_tail_barriers(D)[self.backward]
        s0, st, qv = int(sync[0].item()), int(status[0].item()), int(queue[0].item())
        assert s0 == want, (f"{c.id}: the {which} launch came up short: barrier counter {s0} of {want} (XCD word {int(sync[1].item())}, roles "
                            f"handed out {int(sync[2].item())}); its results are not looked at")
        assert st == 0, f"{c.id}: the {which} launch flagged itself: status word {st}"
        handed = self.form["tiles"] + self.form["tickets"]
        assert qv >= handed, f"{c.id}: the {which} launch handed out {qv} of {handed} rider tiles and shadow tickets"

    def check_riders(self):
        """the riding GEMM: the same bits as mst_gemm_nt on the same arguments, inside the fp64 bound; the shadows: exact"""
        c = self.c
        if self.rider is None:
            return
        ref = self.rider["C"].clone()
        self.o.gemm_nt(**{k: v for k, v in _rider_kw(self.rider, ref).items()})
        torch.cuda.synchronize()
        assert torch.equal(self.C.view(torch.int16), ref.view(torch.int16)), f"{c.id}: the riding GEMM differs from mst_gemm_nt"
        host = T.rider_operands(c, self.backward)
        res, bad = T.rider_check(c, host, self.C.cpu())
        print(f"    rider ({'backward' if self.backward else 'forward'}): worst error / bound {res.ratio:.3f}")
        assert not res.bad.any(), T.describe(c, res)
        assert not bad, "\n".join(bad)
        if self.shadows is not None:
            bad = T.shadow_check(c, self.sh_host, self.wt16.cpu())
            assert not bad, "\n".join(bad)


def _directions(c):
    return [b for b, _ in T.case_forms(c)]


def _run(o, c, ins, gpu, u=None, with_rider=True):
    """the case's launches (forward, then backward for a chain) into fresh outputs, or into u -> (outputs on the device, launches)"""
    i = {k: t.to(gpu) for k, t in ins.items()}
    if u is None:
        u = {k: t.to(gpu) for k, t in T.outputs(c).items()}
    launches = []
    for backward in _directions(c):
        ln = Launch(o, c, backward, gpu, with_rider)
        ln.run(i, u)
        launches.append(ln)
    return u, launches


def _host(u):
    return {k: t.cpu() for k, t in u.items()}


def _same_bits(a, b):
    return [k for k in a if not torch.equal(a[k].view(torch.int16 if a[k].element_size() == 2 else torch.int32),
                                            b[k].view(torch.int16 if b[k].element_size() == 2 else torch.int32))]


def _hold(c, ins, got, what):
    results = T.check(c, ins, got)
    print(f"\n{c.id}{what}: worst error / bound " + ", ".join(f"{r.name} {r.ratio:.3f}" for r in results))
    failed = [T.describe(c, r) for r in results if r.bad.any()]
    assert not failed, "\n".join(failed)
    assert T.intact(c, got) == []


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_row_tail_launch_against_fp64(gpu, case):
    from musicstyletransfer_amd import ops as o
    c = case
    ins = T.operands(c)
    u, launches = _run(o, c, ins, gpu)
    got = _host(u)
    _hold(c, ins, got, "")
    for ln in launches:
        ln.check_riders()
    # two identical launches give identical bits, the parameter gradients (16 waves through LDS, then one atomic each) included
    again = _host(_run(o, c, ins, gpu)[0])
    assert _same_bits(got, again) == [], "not run-to-run identical"
    if c.rider != "none":   # (printed, not asserted: another instantiation of the same chain)
        plain = _host(_run(o, c, ins, gpu, with_rider=False)[0])
        diff = _same_bits(got, plain)
        print(f"    the riding and the plain kernel: {'the same bits' if not diff else 'different bits in ' + ', '.join(diff)}")
    if c.id in T.STALE:
        # other operands into the SAME output buffers (sync words zeroed again, the accumulated parameter gradients set back to their
        # initial value): a row left from the first launch, read because a barrier let a workgroup through early, is now wrong
        bufs, _ = T.plan(c)
        for name, b in bufs.items():
            if b.out and b.rows == "vec":
                u[name][:b.width] = T.INIT
        ins2 = T.operands(c, salt=1)
        assert any(not torch.equal(ins[k], ins2[k]) for k in ins if k != "seed_word")
        u2, _ = _run(o, c, ins2, gpu, u=u)
        _hold(c, ins2, _host(u2), " (second launch, other operands, same buffers)")
