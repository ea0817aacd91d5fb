"""The class-table job of the weight-gradient flush without a GPU: ABI 115 exports it; a bad job is refused before any HIP call, by the
flush and by the launch of its own with the same message; and whether the job rides on the reduction pass or falls back to a launch
is the flush's own plan (mst_gemm_wgrad_plan), for the batches of tests/wgrad_refs.py."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_refs as W  # noqa: E402
from wgrad_refs import Prob  # noqa: E402

P = 1 << 20  # an aligned address that is never followed


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def test_abi_115_exports_the_job(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 115
    flush, cls = _lib.SIGNATURES["mst_gemm_wgrad_batch_flush"][1], _lib.SIGNATURES["mst_gemm_wgrad_batch_flush_cls"][1]
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert cls == flush[:-1] + [vp, vp, vp, i64, i64, i64] + flush[-1:]
    assert _lib.SIGNATURES["mst_class_table_grad"] == (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp])
    assert len(_lib.STRUCTS) == 12  # (scalar arguments only: no new struct; the twelfth is ABI 119's mst_adam_args)


@pytest.mark.parametrize("job,text", [
    ((None, P, P, 256, 64, 256), b"null pointer"), ((P, None, P, 256, 64, 256), b"null pointer"), ((P, P, None, 256, 64, 256), b"null pointer"),
    ((P, P, P, 256, 0, 256), b"must be positive"), ((P, P, P, 256, 64, 0), b"must be positive"), ((P, P, P, 256, -1, 256), b"must be positive"),
    ((P, P, P, 255, 64, 256), b"ld_cls < Dd"), ((P, P, P, 1 << 31, 64, 1 << 30), b"must be positive"),
])
def test_a_bad_job_is_refused_before_any_hip_call(lib, job, text):
    from musicstyletransfer_amd import _lib
    args = W.plan_args([Prob("edge", 256, 72, 64)], W.BF, _lib.WgradArgs)
    arr = (_lib.WgradArgs * 1)(*args)
    assert lib.mst_class_table_grad(*job, None) == -1
    msg = lib.mst_last_error()
    assert text in msg and msg.startswith(b"mst_class_table_grad"), msg
    assert lib.mst_gemm_wgrad_batch_flush_cls(arr, 1, None, 0, None, 0, None, 0, *job, None) == -1 and lib.mst_last_error() == msg


def test_no_job_at_all_is_not_a_launch_of_its_own(lib):
    assert lib.mst_class_table_grad(None, None, None, 0, 0, 0, None) == -1 and b"null pointer" in lib.mst_last_error()


def test_a_bad_batch_is_refused_with_the_flushs_message_whatever_the_job(lib):
    from musicstyletransfer_amd import _lib
    args = W.plan_args([Prob("edge", 256, 72, 64)], W.BF, _lib.WgradArgs, ldw=60)
    arr = (_lib.WgradArgs * 1)(*args)
    assert lib.mst_gemm_wgrad_batch_flush(arr, 1, None, 0, None, 0, None, 0, None) == -1
    msg = lib.mst_last_error()
    assert b"ldw < K" in msg
    assert lib.mst_gemm_wgrad_batch_flush_cls(arr, 1, None, 0, None, 0, None, 0, P, P, P, 256, 64, 256, None) == -1
    assert lib.mst_last_error() == msg
    assert lib.mst_gemm_wgrad_batch_flush_cls(arr, 1, None, 0, None, 0, None, 0, None, None, None, 0, 0, 0, None) == -1
    assert lib.mst_last_error() == msg


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.id)
def test_the_job_rides_exactly_where_the_tiles_take_the_reduction_pass(lib, case):
    """the fallback decision is the plan's: a reduction pass exists for 256 x 256 tiles with a scratch buffer that holds the slabs"""
    from musicstyletransfer_amd import _lib, ops
    args = W.plan_args(case.probs, case.dtype, _lib.WgradArgs)
    rides = ops.flush_jobs_ride(args, case.scratch_bytes)
    assert rides == bool(case.plan.two_pass & 1)
    assert not ops.flush_jobs_ride(args, 0)
    if rides:
        assert case.plan.form == 3 and case.scratch_bytes >= case.plan.items * 256 * 256 * 4


def test_both_outcomes_are_among_the_cases(lib):
    from musicstyletransfer_amd import _lib, ops
    seen = {ops.flush_jobs_ride(W.plan_args(c.probs, c.dtype, _lib.WgradArgs), c.scratch_bytes) for c in W.CASES}
    assert seen == {True, False}
