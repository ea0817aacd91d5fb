"""Piano-roll precision / recall / F1 without a device: engine.roll_scores, the host metric classes, the ABI surface of the counts
(mst_bce_args.counts, mst_sigmoid_bce_counts, MST_ROLL_SLOTS) and the validation of the counts pointer, which comes before any HIP call."""
import ctypes
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def test_roll_scores_known_answers():
    from musicstyletransfer_amd.engine import roll_scores
    # 10 cells: 4 positives, 5 predicted, 3 of them right -> fp 2, fn 1, tn 4
    s = roll_scores(3, 5, 4, 10)
    assert s == dict(precision=3 / 5, recall=3 / 4, f1=6 / 9, cell_acc=7 / 10)
    assert roll_scores(4, 4, 4, 4) == dict(precision=1.0, recall=1.0, f1=1.0, cell_acc=1.0)
    assert roll_scores(0, 3, 2, 5) == dict(precision=0.0, recall=0.0, f1=0.0, cell_acc=0.0)
    # counts beyond 2^53 stay exact ratios of Python ints
    big = 1 << 60
    assert roll_scores(big, 2 * big, 4 * big, 8 * big) == dict(precision=0.5, recall=0.25, f1=2 / 6, cell_acc=0.5)


def test_roll_scores_zero_denominators():
    from musicstyletransfer_amd.engine import roll_scores
    s = roll_scores(0, 0, 4, 10)      # the model predicts silence everywhere
    assert math.isnan(s["precision"]) and s["recall"] == 0.0 and s["f1"] == 0.0 and s["cell_acc"] == 0.6
    s = roll_scores(0, 3, 0, 10)      # no note in the labels
    assert s["precision"] == 0.0 and math.isnan(s["recall"]) and s["f1"] == 0.0 and s["cell_acc"] == 0.7
    s = roll_scores(0, 0, 0, 10)      # neither
    assert math.isnan(s["precision"]) and math.isnan(s["recall"]) and math.isnan(s["f1"]) and s["cell_acc"] == 1.0
    assert all(math.isnan(v) for v in roll_scores(0, 0, 0, 0).values())   # nothing counted (right after a reset)
    assert set(roll_scores(0, 0, 0, 0)) == {"precision", "recall", "f1", "cell_acc"}


def test_host_classes_agree_with_roll_scores():
    from musicstyletransfer_amd.engine import roll_scores
    from musicstyletransfer_amd.VarAutoEncoder import metrics
    rng = np.random.default_rng(5)
    host = [metrics.Precision(), metrics.Recall(), metrics.F1()]
    tp = pred = pos = cells = 0
    for shape in ((3, 7, 30), (2, 5, 36)):  # two updates accumulate
        labels = (rng.random(shape) < 0.2).astype(np.uint8)
        probs = rng.random(shape).astype(np.float32)
        probs[0, 0, :4] = 0.5               # exactly 0.5 is not predicted
        for m in host:
            m.update(labels, probs)
        p = probs > 0.5
        tp, pred, pos, cells = tp + int((p & (labels == 1)).sum()), pred + int(p.sum()), pos + int(labels.sum()), cells + labels.size
    assert 0 < tp < pred and tp < pos
    want = roll_scores(tp, pred, pos, cells)
    got = dict(m.get() for m in host)
    assert got == {k: want[k] for k in ("precision", "recall", "f1")}
    assert [m.name for m in host] == ["precision", "recall", "f1"]
    for m in host:
        m.reset()
        assert math.isnan(m.get()[1])


def test_abi_surface(lib):
    from musicstyletransfer_amd import _lib
    structs, sigs, consts = _lib.parse_header(open(os.path.join(ROOT, "include", "mst_hip.h")).read())
    assert consts["MST_ROLL_SLOTS"] == 256 and _lib.ROLL_SLOTS == 256
    assert _lib.BceArgs._fields_[-1] == ("counts", ctypes.c_void_p)
    assert [f for f, _ in _lib.BceArgs._fields_[:-1]] == ["labels", "T", "label_smoothing", "downweight", "loss", "probs", "ldp", "logits", "ldl",
                                                         "gscale"]
    assert _lib.BceArgs().counts is None    # a caller that does not know the field passes NULL
    res, args = sigs["mst_sigmoid_bce_counts"]
    res0, args0 = sigs["mst_sigmoid_bce"]
    assert res == res0 and args == args0[:-1] + [ctypes.c_void_p, args0[-1]] and len(args) == 19
    assert hasattr(lib, "mst_sigmoid_bce_counts") and lib.mst_version() >= 114


def _bn128_structs():
    from musicstyletransfer_amd import _lib
    A = 1 << 20
    g, q = _lib.GemmArgs(), _lib.BceArgs()
    g.dtype, g.M, g.N, g.K = 0, 128, 128, 64
    g.A, g.lda, g.B, g.ldb, g.bias, g.alpha, g.C, g.ldc = A, 64, 2 * A, 64, 3 * A, 1.0, 4 * A, 128
    q.labels, q.T, q.loss, q.gscale = 5 * A, 64, 6 * A, 1.0
    return g, q


@pytest.mark.parametrize("off", [8, 4, 1])
def test_a_misaligned_counts_pointer_is_refused_before_any_hip_call(lib, off):
    g, q = _bn128_structs()
    form = (ctypes.c_int64 * 4)()
    q.counts = 7 << 20
    assert lib.mst_gemm_sigmoid_bce_form(ctypes.byref(g), ctypes.byref(q), None, None, form) == 0 and list(form)[:3] == [128, 1, 0]
    q.counts = (7 << 20) + off
    rc = lib.mst_gemm_sigmoid_bce_form(ctypes.byref(g), ctypes.byref(q), None, None, form)
    msg = lib.mst_last_error()
    assert rc == -1 and b"counts must be 16-byte aligned" in msg, (rc, msg)
    assert lib.mst_gemm_sigmoid_bce(ctypes.byref(g), ctypes.byref(q), None) == -1 and lib.mst_last_error() == msg
    # the unfused launch: the same refusal
    A = 1 << 20
    a = (0, 2, 64, 128, A, 128, 2 * A, 0.0, 0, None, 3 * A, None, 0, None, 0, 1.0, 0)
    assert lib.mst_sigmoid_bce_counts(*a, (7 << 20) + off, None) == -1 and b"counts must be 16-byte aligned" in lib.mst_last_error()


def test_ops_refuse_a_counts_buffer_of_the_wrong_kind():
    import torch
    from musicstyletransfer_amd import _lib, ops
    for bad in (torch.zeros(_lib.ROLL_SLOTS, 4, dtype=torch.int32), torch.zeros(_lib.ROLL_SLOTS, 3, dtype=torch.int64),
                torch.zeros(4, _lib.ROLL_SLOTS, dtype=torch.int64).t()):
        with pytest.raises(AssertionError):
            ops._roll_counts(bad)
    assert ops._roll_counts(None) is None
