"""mst_kqv_ffn_ln_bwd without a GPU: ABI 116 exports the launch and its form query; every argument check of the new entry point fires
before any HIP call, with its message; and the form query — the one rule that says where the K | Q | V input gradient runs as the head of
the feed-forward backward launch — answers for the shapes tests/test_ffn_ln_bwd_head_gpu.py runs and refuses what the head cannot take."""
import ctypes as C

import pytest

P = 1 << 20  # an aligned address that is never followed
BF, FP = 0, 1


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def _args(M=1792, D=256, dtype=BF, store=True, p=0.1):
    """valid arguments of the one-launch form: (head, lead, ff2_dgrad, ff1_dgrad, ln)"""
    from musicstyletransfer_amd import _lib
    F = 4 * D

    def gemm(m, n, k, lda, ldb, ldc):
        g = _lib.GemmArgs()
        g.dtype, g.M, g.N, g.K, g.alpha = dtype, m, n, k, 1.0
        g.A, g.lda, g.B, g.ldb, g.C, g.ldc = P, lda, 2 * P, ldb, 3 * P, ldc
        return g

    head = gemm(M, D, 3 * D, 3 * D, 3 * D, D)
    head.resid, head.ldr = 4 * P, D
    if not store:
        head.C, head.ldc = None, 0
    lead = _lib.LnBwdIn()
    lead.dy, lead.ld_dy = head.C, head.ldc
    lead.x, lead.ld_x, lead.gamma, lead.mean, lead.rstd = 5 * P, D, 6 * P, 7 * P, 8 * P
    lead.dx, lead.ld_dx, lead.dx_masked, lead.ld_dxm, lead.partials = 9 * P, D, 10 * P, D, 11 * P
    lead.mask_mode, lead.dropout_p = 1, p
    g1 = gemm(M, F, D, D, D, F)
    g1.A, g1.C, g1.gate, g1.ldg = lead.dx_masked, 12 * P, 13 * P, F
    g2 = gemm(M, D, F, F, F, D)
    g2.A, g2.C, g2.resid, g2.ldr = g1.C, 14 * P, lead.dx, D
    ln = _lib.LnArgs()
    ln.mode, ln.gamma, ln.mean, ln.rstd, ln.x, ln.ld_x, ln.partials = 2, 15 * P, 16 * P, 17 * P, 18 * P, D, 19 * P
    return head, lead, g1, g2, ln


def _call(lib, a, drop=None):
    ptrs = [None if i == drop else C.byref(x) for i, x in enumerate(a)]
    return lib.mst_kqv_ffn_ln_bwd(*ptrs, None)


def _form(lib, a):
    form = (C.c_int64 * 1)(-7)
    rc = lib.mst_kqv_ffn_ln_bwd_form(C.byref(a[0]), C.byref(a[2]), C.byref(a[3]), form)
    return rc, form[0]


def test_abi_116_exports_the_launch_and_its_form_query(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 116
    g, q, l = (C.POINTER(_lib.STRUCTS[n]) for n in ("mst_gemm_args", "mst_ln_bwd_in", "mst_ln_args"))
    assert _lib.SIGNATURES["mst_kqv_ffn_ln_bwd"] == (C.c_int, [g, q, g, g, l, C.c_void_p])
    assert _lib.SIGNATURES["mst_kqv_ffn_ln_bwd_form"] == (C.c_int, [g, g, g, C.c_void_p])
    assert len(_lib.STRUCTS) == 12  # (the head is an mst_gemm_args: no new struct; the twelfth is ABI 119's mst_adam_args)


def _mut(**fields):
    def f(a):
        for k, v in fields.items():
            who, name = k.split("__")
            setattr(a[dict(head=0, lead=1, ff2=2, ff1=3, ln=4)[who]], name, v)
    return f


@pytest.mark.parametrize("change,drop,text", [
    (None, 0, b"null args"), (None, 2, b"null args"), (None, 3, b"null args"), (None, 1, b"null args"), (None, 4, b"null args"),
    (_mut(head__M=0), None, b"the head's M,N,K must be positive (got 0,256,768)"),
    (_mut(head__K=-8), None, b"the head's M,N,K must be positive"),
    (_mut(head__A=None), None, b"the head's A and B operands are missing"),
    (_mut(head__B=None), None, b"the head's A and B operands are missing"),
    (_mut(head__M=1728), None, b"the head's result is the block's incoming gradient: M x width (got 1728 x 256)"),
    (_mut(head__N=128), None, b"the head's result is the block's incoming gradient"),
    (_mut(lead__dy=21 * P), None, b"lead->dy is the head's C"),
    (_mut(lead__ld_dy=264), None, b"lead->dy is the head's C"),
    (_mut(head__C=None, lead__dy=None, head__bias=20 * P), None, b"this shape runs the GEMM launch first and needs the head's C"),
    (_mut(head__C=None, lead__dy=None, head__ldr=260), None, b"this shape runs the GEMM launch first and needs the head's C"),
])
def test_every_new_check_fires_before_any_hip_call(lib, change, drop, text):
    a = _args()
    if change:
        change(a)
    assert _call(lib, a, drop) == -1
    msg = lib.mst_last_error()
    assert msg.startswith(b"mst_kqv_ffn_ln_bwd:") and text in msg, msg


def test_the_parts_keep_their_own_checks(lib):
    """the block's arguments are checked as mst_ffn_ln_bwd_lead checks them, in both forms, under the new entry point's name; in the
    two-launch form the GEMM's own check speaks before anything is launched"""
    for bias in (None, 20 * P):  # one launch / two launches
        a = _args()
        a[0].bias = bias
        a[4].gamma = None
        assert _call(lib, a) == -1
        assert lib.mst_last_error().startswith(b"mst_kqv_ffn_ln_bwd: LayerNorm arguments of the wrong form")
        a = _args()
        a[0].bias = bias
        a[1].x = None
        assert _call(lib, a) == -1 and b"mst_kqv_ffn_ln_bwd: leading LayerNorm: null pointer" in lib.mst_last_error()
    a = _args()
    a[0].ldr = 258  # (not a multiple of 4: mst_gemm_nt refuses it)
    assert _call(lib, a) == -1 and b"mst_gemm_nt: ldr" in lib.mst_last_error()
    a = _args(store=False)
    a[1].dy = None
    a[1].x = None  # the one-launch form without a stored gradient still checks the lead
    assert _call(lib, a) == -1 and b"leading LayerNorm: null pointer" in lib.mst_last_error()


@pytest.mark.parametrize("dtype", (BF, FP))
@pytest.mark.parametrize("D", (256, 128))
@pytest.mark.parametrize("M", (28 * 64, 8 * 64, 3 * 64, 28 * 64 - 17, 4 * 64, 16384))
@pytest.mark.parametrize("store", (True, False))
def test_the_form_query_takes_the_shapes_the_gpu_tests_run(lib, dtype, D, M, store):
    assert _form(lib, _args(M, D, dtype, store)) == (0, 1)


@pytest.mark.parametrize("change", [
    _mut(head__N=64, head__K=192, head__lda=192, head__ldb=192, ff1__N=64, ff2__K=64, ff2__N=256, ff1__K=256),  # width 64
    _mut(head__K=512), _mut(head__K=1024, head__lda=1024, head__ldb=1024),  # K != 3 x width
    _mut(head__resid=4 * P + 8), _mut(head__ldr=260), _mut(head__C=3 * P + 8, lead__dy=3 * P + 8),  # operands the 16-byte accesses cannot take
    _mut(head__ldc=260, lead__ld_dy=260), _mut(head__lda=760), _mut(head__ldb=512),
    _mut(head__resid=None), _mut(head__bias=20 * P), _mut(head__alpha=0.5), _mut(head__gate=20 * P, head__ldg=256), _mut(head__act=1),
    _mut(head__dropout_p=0.1), _mut(head__self_resid=1), _mut(head__c_f32=1), _mut(head__a_u8=1),
    _mut(head__a_rows_per_group=64, head__a_group_stride=128), _mut(head__c_rows_per_group=64, head__c_group_stride=128),
    _mut(ff2__a_rows_per_group=64, ff2__a_group_stride=128), _mut(head__dtype=FP),
])
def test_the_form_query_refuses_what_the_head_cannot_take(lib, change):
    a = _args()
    change(a)
    assert _form(lib, a) == (0, 0)


def test_the_form_query_checks_its_own_arguments(lib):
    a = _args()
    assert lib.mst_kqv_ffn_ln_bwd_form(C.byref(a[0]), C.byref(a[2]), C.byref(a[3]), None) == -1 and b"null form" in lib.mst_last_error()
    assert lib.mst_kqv_ffn_ln_bwd_form(None, C.byref(a[2]), C.byref(a[3]), (C.c_int64 * 1)()) == -1 and b"null args" in lib.mst_last_error()
    a[0].M = 64
    assert _form(lib, a)[0] == -1 and lib.mst_last_error().startswith(b"mst_kqv_ffn_ln_bwd_form: the head's result is the block's")


def test_the_engine_rule_follows_the_library(lib):
    """ops.kqv_head_pays asks the library with stand-in arguments of the engine's own layout"""
    import torch
    from musicstyletransfer_amd import ops
    for dtype in (torch.bfloat16, torch.float16):
        assert ops.kqv_head_pays(dtype, 16384, 256) and ops.kqv_head_pays(dtype, 256, 128)
        assert not ops.kqv_head_pays(dtype, 16384, 64) and not ops.kqv_head_pays(dtype, 16384, 512)
