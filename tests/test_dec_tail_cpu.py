"""mst_dec_tail_step without a GPU: the entry point refuses every shape it was not built for before any HIP call, with a message that
names the reason; ops.dec_tail_pays answers from the shape alone."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


B, T, D, F, P = 2, 64, 128, 512, 128
M, R = B * T, B * (T + 1)


def _addr(k):
    return 0x100000 * (k + 1)  # (never dereferenced: validation reads the structs only)


def _gemm(A, Bm, Cm, N, K, lda, ldc, a_groups=False, c_groups=False):
    from musicstyletransfer_amd import _lib
    g = _lib.GemmArgs()
    g.dtype, g.M, g.N, g.K = _lib.MST_BF16, M, N, K
    g.A, g.lda, g.B, g.ldb, g.C, g.ldc = A, lda, Bm, K, Cm, ldc
    g.alpha = 1.0
    if a_groups:
        g.a_rows_per_group, g.a_group_stride, g.a_group_offset = T, T + 1, 1
    if c_groups:
        g.c_rows_per_group, g.c_group_stride, g.c_group_offset = T, T + 1, 1
    return g


def _ln(mode, out=None, x=None, mask_mode=0):
    from musicstyletransfer_amd import _lib
    l = _lib.LnArgs()
    l.mode, l.gamma, l.beta, l.eps = mode, _addr(30), _addr(31), 1e-5
    l.mean, l.rstd = _addr(32), _addr(33)
    l.out, l.ld_out = out, (D if out else 0)
    l.x, l.ld_x = x, (D if x else 0)
    l.partials, l.mask_mode = (_addr(34) if mode == 2 else None), mask_mode
    return l


def _parts():
    """the twelve structs of a call the entry point would launch (configs[1]'s shape at B 2, T 64)"""
    from musicstyletransfer_amd import _lib
    att, h1, x1, a, h2, x2, dl, dh, dpre, dh1 = (_addr(k) for k in range(10))
    proj = _gemm(att, _addr(10), h1, D, D, D, D)
    ln1 = _ln(1, out=x1)
    ff1 = _gemm(x1, _addr(11), a, F, D, D, F, a_groups=True)
    ff1.act = _lib.ACT_RELU
    ff2 = _gemm(a, _addr(12), h2, D, F, F, D)
    ff2.self_resid = 1
    ln3 = _ln(1, out=x2)
    out = _gemm(x2, _addr(13), dl, P, D, D, P, a_groups=True)
    bce = _lib.BceArgs()
    bce.labels, bce.T, bce.loss, bce.gscale = _addr(14), T, _addr(15), 1.0
    odg = _gemm(dl, _addr(16), dh, D, P, P, D, c_groups=True)
    ln3b = _ln(2, x=h2, mask_mode=2)
    f2d = _gemm(dh, _addr(17), dpre, F, D, D, F, a_groups=True)
    f2d.gate, f2d.ldg = a, F
    f1d = _gemm(dpre, _addr(18), dh1, D, F, F, D)
    ln1b = _ln(2, x=h1)
    return dict(proj=proj, ln1=ln1, ff1=ff1, ff2=ff2, ln3=ln3, out=out, bce=bce, out_dgrad=odg, ln3_bwd=ln3b, ff2_dgrad=f2d,
                ff1_dgrad=f1d, ln1_bwd=ln1b)


def _call(lib, parts):
    return lib.mst_dec_tail_step(*(ctypes.byref(p) for p in parts.values()), None)


def _set(parts, path, value):
    name, field = path.split(".")
    setattr(parts[name], field, value)


@pytest.mark.parametrize("edits,message", [
    ({"ff2.N": 256, "ff1.K": 256}, b"model width must be 128"),
    ({"ff1.N": 1024, "ff2.K": 1024, "ff2_dgrad.N": 1024}, b"hidden width must be 512"),
    ({"out.N": 256}, b"128 pitches"),
    ({"bce.T": 96}, b"T must be a multiple of 64"),
    ({"out.M": M - 32}, b"whole 64-row tiles"),
    ({"ff1.M": M + 64}, b"whole 64-row tiles"),
    ({"ff1.a_group_offset": 0}, b"row groups must be (T, T + 1, 1)"),
    ({"out.a_rows_per_group": 0}, b"row groups must be (T, T + 1, 1)"),
    ({"out_dgrad.c_group_stride": T}, b"row groups must be (T, T + 1, 1)"),
    ({"ff2_dgrad.a_rows_per_group": 0}, b"row groups must be (T, T + 1, 1)"),
    ({"ln3_bwd.mask_mode": 1}, b"mask mode 2"),
    ({"ln3_bwd.mask_mode": 0}, b"mask mode 2"),
    ({"out.A": _addr(40)}, b"LayerNorm-3's output"),
    ({"out_dgrad.A": _addr(41)}, b"logit gradient"),
    ({"ff2_dgrad.A": _addr(42)}, b"output dgrad's dX_out"),
    ({"ff2_dgrad.gate": None}, b"gate"),             # (the parts' own checks follow the shape's)
    ({"bce.labels": None}, b"labels"),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_unsupported_shapes_are_refused_before_any_hip_call(lib, edits, message):
    parts = _parts()
    for path, value in edits.items():
        _set(parts, path, value)
    assert _call(lib, parts) == -1
    err = lib.mst_last_error()
    assert err.startswith(b"mst_dec_tail_step:") or message in (b"gate", b"labels"), err
    assert message in err, err


def test_null_struct_is_refused(lib):
    parts = _parts()
    args = [ctypes.byref(p) for p in parts.values()]
    args[5] = None
    assert lib.mst_dec_tail_step(*args, None) == -1
    assert b"null args" in lib.mst_last_error()


def test_dec_tail_pays():
    from musicstyletransfer_amd import ops as o
    assert o.dec_tail_pays(128, 512, 128, 256, 64 * 256 // 64, 256)        # configs[1]: 256 tiles, one resident round
    assert not o.dec_tail_pays(128, 512, 2048, 256, 64 * 256 // 64, 256)   # configs[2]: 2048 pitches, no fused loss launch
    assert not o.dec_tail_pays(128, 512, 128, 1024, 32 * 1024 // 64, 256)  # configs[4]: 512 tiles on 256 compute units
    assert not o.dec_tail_pays(128, 512, 293, 64, 8, 256)                  # token path: a vocabulary, not 128 pitches
    assert not o.dec_tail_pays(256, 1024, 128, 256, 256, 256)              # width 256
    assert not o.dec_tail_pays(128, 512, 128, 33, 2, 256)                  # T not in whole tiles
    assert o.dec_tail_pays(128, 512, 128, 64, 3, 256)
