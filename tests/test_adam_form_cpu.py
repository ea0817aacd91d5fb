"""mst_adam_flat_form: what one mst_adam_args block launches — the kernel's three switches, the transposed shadows kept, the step-count
launch ahead — over every combination of the optional groups, and every refusal of the launch with the launch's status and message. No
HIP call on either side: the form query and the launch decide with the same host function."""
import ctypes as C
import itertools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ONE = 16  # a non-NULL, 16-byte aligned stand-in for a device buffer: neither entry point follows it


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _block(lib, sched=False, gnorm=False, ema=False, n_emb=0, tick=False, **kw):
    from musicstyletransfer_amd import _lib
    q = _lib.AdamArgs(dtype=_lib.MST_BF16, n=1000, w=ONE, grad=ONE, m=ONE, v=ONE, w16=ONE, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                      rescale=1.0, clip=-1.0, step_state=ONE, advance_step=1 if tick else 0)
    if sched:
        q.sched = ONE
    if gnorm:
        q.parts, q.n_parts, q.max_norm, q.gstat = ONE, lib.mst_grad_sumsq_parts(), 1.0, ONE
    if ema:
        q.ema, q.decay = ONE, 0.99
    if n_emb:
        q._emb = (C.c_int64 * 8)(0, 0, 8, 16, 500, 128, 5, 7)  # {source offset, offset in wt16, rows, cols} of two matrices
        q.base, q.emb, q.n_emb, q.wt16 = 256, C.addressof(q._emb), n_emb, ONE
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _form(lib, q):
    form = (C.c_int64 * 6)(*([-7] * 6))
    rc = lib.mst_adam_flat_form(q, form)
    return rc, list(form)


def test_form_reports_exactly_the_switches_of_the_block(lib):
    from musicstyletransfer_amd import _lib
    seen = set()
    for sched, gnorm, ema in itertools.product((False, True), repeat=3):
        for n_emb in (0, 1, 2):
            for tick in (False, True):
                q = _block(lib, sched, gnorm, ema, n_emb, tick)
                rc, form = _form(lib, q)
                if tick and (sched or gnorm or ema or n_emb):  # the step count of these groups is mst_step_begin's
                    assert rc == -1 and b"advance_step" in lib.mst_last_error() and form == [-7] * 6
                    continue
                assert rc == 0, lib.mst_last_error()
                assert form == [int(sched), int(gnorm), int(ema), n_emb, int(tick), -7], (sched, gnorm, ema, n_emb, tick)
                seen.add(tuple(form[:5]))
                q.dtype = _lib.MST_F16  # the same form for the other activation type
                assert _form(lib, q) == (0, form)
    assert len(seen) == 8 * 3 + 1
    # gstat, metrics and w16 are no switches
    for kw in (dict(gstat=None), dict(w16=None), dict(metrics=C.pointer(_lib.StepMetrics()))):
        assert _form(lib, _block(lib, True, True, True, 2, **kw)) == (0, [1, 1, 1, 2, 0, -7])
    # emb without matrices (n_emb = 0) keeps none
    q = _block(lib, n_emb=2)
    q.n_emb = 0
    assert _form(lib, q) == (0, [0, 0, 0, 0, 0, -7])


def _refusals(lib):
    """(the fields of a refused block, the status, a fragment of the message), in the order of the launch's checks"""
    from musicstyletransfer_amd import _lib
    G = lib.mst_grad_sumsq_parts()
    nan, inf = float("nan"), float("inf")
    bad_mt = _lib.StepMetrics(recon=ONE)  # (B = 0, no kl)
    no_status = _lib.StepMetrics(expect_ptr0=ONE)
    full = dict(sched=True, gnorm=True, ema=True, n_emb=2)
    cases = [
        (dict(ema=False, decay=0.5), -1, b"without ema"), (dict(ema=False, decay=nan), -1, b"without ema"),
        (dict(ema=True, **{"ema_": 20}), -1, b"ema must be 16-byte aligned"),
        *[(dict(ema=True, decay=d), -1, b"decay must lie in (0, 1)") for d in (0.0, -0.5, 1.0, 2.0, inf, nan)],
        (dict(n_parts=G), -1, b"without parts"), (dict(max_norm=1.0), -1, b"without parts"), (dict(gstat=ONE), -1, b"without parts"),
        (dict(gnorm=True, parts=20), -1, b"parts must be 16-byte aligned"),
        (dict(gnorm=True, n_parts=G - 1), -1, b"mst_grad_sumsq_parts() = %d" % G), (dict(gnorm=True, n_parts=0), -1, b"mst_grad_sumsq_parts"),
        *[(dict(gnorm=True, max_norm=x), -1, b"max_norm must be positive and finite") for x in (0.0, -1.0, inf, nan)],
        (dict(n_emb=1, **{"n_emb_": 3}), -1, b"up to two matrices"), (dict(n_emb=1, **{"n_emb_": -1}), -1, b"up to two matrices"),
        (dict(n_emb=1, wt16=None), -1, b"up to two matrices"), (dict(n_emb=1, emb=None), -1, b"up to two matrices"),
        (dict(n_emb=1, base=-8), -1, b"up to two matrices"),
        (dict(n_emb=2, rows1=0), -1, b"bad matrix 1"), (dict(n_emb=2, rows0=1 << 16, cols0=1 << 15), -1, b"bad matrix 0"),
        (dict(n_emb=1, dst0=-1), -1, b"bad matrix 0"),
        *[(dict(tick=True, **{k: True if k != "n_emb" else 1}), -1, b"advance_step") for k in ("sched", "gnorm", "ema", "n_emb")],
        (dict(n=0), -1, b"mst_adam_flat: bad argument"),
        *[(dict(full, **{k: None}), -1, b"mst_adam_flat: bad argument") for k in ("w", "grad", "m", "v", "step_state")],
        (dict(metrics=C.pointer(bad_mt)), -1, b"metrics need B, recon and kl"),
        (dict(metrics=C.pointer(no_status)), -1, b"expectations need the status words"),
        *[(dict(full, **{k: 24}), -1, b"buffers must be 16-byte aligned") for k in ("w", "grad", "m", "v")],
        (dict(full, dtype=_lib.MST_F32), -3, b"unsupported activation dtype"), (dict(dtype=7), -3, b"unsupported activation dtype"),
    ]
    return cases


def test_every_refusal_is_the_launchs_in_status_and_message(lib):
    for kw, status, fragment in _refusals(lib):
        kw = dict(kw)
        mats = {k: kw.pop(k) for k in list(kw) if k[:-1] in ("rows", "cols", "dst")}
        late = {k[:-1]: kw.pop(k) for k in list(kw) if k.endswith("_")}  # (fields set over what _block derives from the switches)
        q = _block(lib, **kw)
        for k, v in mats.items():
            q._emb[4 * int(k[-1]) + {"dst": 1, "rows": 2, "cols": 3}[k[:-1]]] = v
        for k, v in late.items():
            setattr(q, k, v)
        rc, form = _form(lib, q)
        said = lib.mst_last_error()
        assert rc == status and fragment in said and said.startswith(b"mst_adam_flat:") == (status == -1), (kw, mats, late, rc, said)
        assert form == [-7] * 6  # nothing written
        # the launch: the same status, the same words (refused before any HIP call: no device is needed to ask)
        assert lib.mst_adam_flat(q, None) == status and lib.mst_last_error() == said, (kw, mats, late)
    # the two of the entry points themselves
    assert lib.mst_adam_flat_form(None, (C.c_int64 * 5)()) == -1 and b"mst_adam_flat: null args" in lib.mst_last_error()
    assert lib.mst_adam_flat(None, None) == -1 and b"mst_adam_flat: null args" in lib.mst_last_error()
    assert lib.mst_adam_flat_form(_block(lib), None) == -1 and b"null form" in lib.mst_last_error()


def test_the_order_of_the_checks(lib):
    """a block wrong in every group is refused for the first of them: ema, parts, the matrices, advance_step, the launch's own"""
    q = _block(lib, gnorm=True, ema=True, n_emb=1, tick=True, n=0, decay=1.0, max_norm=0.0, base=-1)
    for fix, fragment in ((dict(decay=0.5), b"decay"), (dict(max_norm=1.0), b"max_norm"), (dict(base=0), b"up to two matrices"),
                          (dict(advance_step=0), b"advance_step"), (dict(n=8), b"bad argument")):
        rc, _ = _form(lib, q)
        assert rc == -1 and fragment in lib.mst_last_error(), (fragment, lib.mst_last_error())
        for k, v in fix.items():
            setattr(q, k, v)
    assert _form(lib, q) == (0, [0, 1, 1, 1, 0, -7])


def test_ops_adam_flat_form_names_the_fields(lib):
    from musicstyletransfer_amd import ops as o
    assert o.adam_flat_form(_block(lib, sched=True, n_emb=2)) == dict(sched=1, gnorm=0, ema=0, emb=2, tick=0)
    assert o.adam_flat_form(C.byref(_block(lib, gnorm=True, ema=True, n_emb=1))) == dict(sched=0, gnorm=1, ema=1, emb=1, tick=0)
    assert o.adam_flat_form(_block(lib, tick=True)) == dict(sched=0, gnorm=0, ema=0, emb=0, tick=1)
    from musicstyletransfer_amd import _lib
    with pytest.raises(_lib.MstError, match="advance_step"):
        o.adam_flat_form(_block(lib, sched=True, tick=True))
