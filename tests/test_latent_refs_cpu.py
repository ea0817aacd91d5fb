"""The latent block without a GPU: the cases of tests/latent_refs.py get the launch form they record (asked of mst_latent_form, the
launches' own decision) and between them reach every value of every form entry; the preloaded forms' boundaries sit where the
kernels' shape functions put them; bad shapes are refused with the launch's own message; the integer operands are exact in fp32 and
in 16 bits; and the staged bounds accept an fp32 evaluation in the two summation orders furthest apart and refuse eleven wrong
kernels (and a KL sum that lost one term)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_refs as R  # noqa: E402

ALIGNED = 4096  # a pointer value for the queries and the refused launches: never followed


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def form_of(c):
    from musicstyletransfer_amd import ops
    if isinstance(c, R.Fwd):
        return tuple(ops.latent_form(c.De, c.Z, c.Dd, c.nq, ALIGNED, part="fwd").values())
    return tuple(ops.latent_form(c.De, c.Z, c.Dd, c.nq, ALIGNED + 4 * c.wl_off, part="bwd").values())


def by_name(table, name):
    return next(c for c in table if c.name == name)


# ------------------------------------------------------------------------------------------ the cases get their forms
def test_abi_108_exports_the_form_query(lib):
    from musicstyletransfer_amd import _lib
    assert lib.mst_version() >= 108
    assert len(_lib.SIGNATURES["mst_latent_form"][1]) == 6


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_every_case_gets_the_form_it_records(lib, c):
    """fails when a limit moves and a case silently runs another kernel"""
    assert form_of(c) == c.form, c.id
    assert c.form == (R.fwd_form(c.De, c.Z, c.Dd, c.nq) if isinstance(c, R.Fwd) else R.bwd_form(c.De, c.Z, c.Dd, c.wl_off)), "the restatement"
    assert c.B <= 8 or c.name.startswith("cls-")


def test_the_cases_reach_every_value_of_every_entry(lib):
    fwd, bwd = {form_of(c)[:4] for c in R.FWD}, {form_of(c)[:2] for c in R.BWD}
    assert {f[0] for f in fwd} == {0, 1} and {f[1] for f in fwd} == {0, 1, 2} and {f[2] for f in fwd} == {0, 1, 2}
    assert {f[3] for f in fwd} == {0, 1, 2, 4}
    assert {(f[0], f[3]) for f in fwd} >= {(1, 2), (0, 2)}, "the projection at Dd 128 both preloaded and general"
    assert bwd == {(1, 0), (0, 1), (0, 2)}
    # ... with a projection in each backward kernel, with and without the residual row, at both widths
    assert {(form_of(c)[0], c.nq, c.resid) for c in R.BWD if c.nq} >= {(1, 384, True), (0, 384, False), (0, 768, False), (0, 768, True)}
    assert sum(c.sched for c in R.BWD) == 3 and {form_of(c)[:2] for c in R.BWD if c.sched} == bwd
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    # the form is a property of the shape: the same for both activation types (the query takes none)
    assert {c.ncls for c in R.BWD if c.name.startswith("cls-")} == {1, 2, 5, 9}
    assert {c.B for c in R.BWD if c.name.startswith("cls-")} == {1, 3, 5, 64, 70}


def test_preloaded_boundaries_sit_where_the_shape_functions_put_them(lib):
    from musicstyletransfer_amd import ops
    f = lambda De, Z, Dd: ops.latent_form(De, Z, Dd)  # noqa: E731
    assert f(256, 64, 128)["fwd_pre"] == 1
    for shape in ((257, 64, 128), (256, 65, 128), (256, 64, 129)):
        assert f(*shape)["fwd_pre"] == 0, shape
    for shape in ((255, 64, 128), (256, 63, 128), (256, 64, 127)):
        assert f(*shape)["fwd_pre"] == 1, shape
    # backward: ceil(Dd / (1024 / Z)) <= 8 and ceil(2 Z / (1024 / De)) <= 32
    assert f(256, 64, 128)["bwd_pre"] == 1
    for shape in ((257, 64, 128), (256, 65, 128), (256, 64, 129)):
        assert f(*shape)["bwd_pre"] == 0, shape
    assert f(1024, 16, 128)["bwd_pre"] == 1 and f(1024, 17, 128)["bwd_pre"] == 0 and f(1025, 16, 128)["bwd_pre"] == 0
    assert f(64, 128, 64)["bwd_pre"] == 1 and f(64, 129, 64)["bwd_pre"] == 0 and f(64, 128, 65)["bwd_pre"] == 0
    # loaders: wave_dots_pre up to four chunks of 64
    assert (f(300, 256, 128)["loader_l"], f(300, 256, 128)["loader_h"]) == (2, 1)
    assert (f(256, 257, 128)["loader_l"], f(256, 257, 128)["loader_h"]) == (1, 2)
    # dh0: four columns while De is whole quads, at most 1024 of them, and Wl is 16-byte aligned
    assert f(4096, 40, 64)["dh0"] == 1 and f(4100, 40, 64)["dh0"] == 2 and f(4098, 40, 64)["dh0"] == 2
    assert [ops.latent_form(256, 256, 128, 0, ALIGNED + off)["dh0"] for off in (0, 4, 8, 12, 16)] == [1, 2, 2, 2, 1]
    assert ops.latent_form(256, 64, 128, 0, ALIGNED + 4)["dh0"] == 0, "the preloaded form does not look at the alignment"
    # the whole grid against the restatement
    for De in (1, 63, 64, 200, 256, 257, 1024, 1025, 1030):
        for Z in (1, 16, 33, 64, 65, 256, 257, 1024):
            for Dd in (1, 64, 100, 128, 129, 256):
                for nq in (0, 3 * Dd if Dd in (128, 256) else 0):
                    got = tuple(f(De, Z, Dd).values()) if not nq else tuple(ops.latent_form(De, Z, Dd, nq).values())
                    assert got == R.fwd_form(De, Z, Dd, nq) + R.bwd_form(De, Z, Dd), (De, Z, Dd, nq)


def test_bad_shapes_are_refused_with_the_launchs_own_message(lib):
    """validation comes before any HIP call in the launches too: same status, same message"""
    P = ALIGNED
    form = (ctypes.c_int64 * 8)(*([-1] * 8))

    def query(De, Z, Dd, nq, text):
        for i in range(8):
            form[i] = -1
        assert lib.mst_latent_form(De, Z, Dd, nq, P, form) == -1
        msg = lib.mst_last_error()
        assert text in msg, msg
        return msg

    def fwd(De, Z, Dd, nq):
        head = (0, 2, De, Z, Dd, P, De, P, P, P, P, P, P, P, Dd, P, 1.0, P, P, P, P, P, Dd)
        return lib.mst_latent_fwd_proj(*head, P, Dd, P, P, nq, nq, None) if nq else lib.mst_latent_fwd(*head, None)

    def bwd(De, Z, Dd, nq):
        head, tail = (0, 2, De, Z, Dd, P, P, P, P, P, P), (1.0, 1.0, 1.0, 1.0, P, Dd, P, De, P, None)
        return lib.mst_latent_bwd_vec_proj(*head, P, nq, P, nq, nq, None, 0, *tail) if nq else lib.mst_latent_bwd_vec(*head, P, Dd, *tail)

    msg = query(64, 1025, 32, 0, b"latent size above 1024")
    assert list(form[:5]) == list(R.fwd_form(64, 1025, 32)) and form[5] == -1, "the forward launch takes Z 1025"
    assert bwd(64, 1025, 32, 0) == -1 and lib.mst_last_error() == msg
    assert lib.mst_latent_form(64, 1024, 32, 0, P, form) == 0
    for Dd in (32, 100, 192, 512):
        msg = query(64, 16, Dd, 3 * Dd, b"decoder width of 64, 128 or 256")
        assert form[0] == -1
        assert fwd(64, 16, Dd, 3 * Dd) == -1 and lib.mst_last_error() == msg
    for Dd, nq in ((64, 192), (128, 200), (128, 383), (256, 384 + 768)):
        msg = query(64, 16, Dd, nq, b"must have 384 or 768 outputs")
        assert list(form[:5]) == list(R.fwd_form(64, 16, Dd, nq)) and form[5] == -1, "the forward projection takes any nq"
        assert bwd(64, 16, Dd, nq) == -1 and lib.mst_last_error() == msg
    msg = query(14000, 334, 64, 0, b"De + 3Z too large")                     # 15002 floats: 60008 bytes
    assert fwd(14000, 334, 64, 0) == -1 and lib.mst_last_error() == msg
    assert lib.mst_latent_form(14000, 333, 64, 0, P, form) == 0 and form[4] == 59996
    msg = query(14000, 200, 128, 384, b"De + 3Z too large")                   # the projection's row and bias count: 15112 floats
    assert fwd(14000, 200, 128, 384) == -1 and lib.mst_last_error() == msg
    assert lib.mst_latent_form(14000, 200, 128, 0, P, form) == 0
    query(0, 16, 64, 0, b"sizes must be positive")
    query(64, 16, 64, -1, b"decoder width of 64, 128 or 256")
    assert lib.mst_latent_form(64, 16, 64, 0, P, None) == -1 and b"null form" in lib.mst_last_error()
    from musicstyletransfer_amd import _lib, ops
    with pytest.raises(_lib.MstError, match="latent size above"):
        ops.latent_form(64, 1025, 32)
    assert ops.latent_form(64, 1025, 32, part="fwd")["fwd_pre"] == 0


# ------------------------------------------------------------------------------------------ operands
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
def test_real_operands_keep_sigma_away_from_zero(dtype):
    for c in R.CASES:
        o = R.operands(c, dtype, "real")
        s = np.abs(R.run(c, o, dtype, prec=np.float64)["sigma"] if isinstance(c, R.Fwd) else o["sigma"])
        assert 2.0 ** -6 <= s.min() and s.max() <= 4.0, (c.id, s.min(), s.max())
        sg = R.run(c, o, dtype, prec=np.float64)["sigma"] if isinstance(c, R.Fwd) else o["sigma"]
        assert (sg > 0).any() and (sg < 0).any(), c.id


def fits32(x):
    return np.array_equal(np.asarray(x, np.float32).astype(np.float64), x)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_integer_mode_is_exact_in_fp32_and_in_16_bits(c, dtype):
    o = R.operands(c, dtype, "int")
    want = R.run(c, o, dtype, prec=np.float64)
    a = o["alpha"]
    assert a == 2.0
    if isinstance(c, R.Fwd):
        exact = R.FWD_EXACT
        assert set(np.unique(np.abs(want["sigma"]))) <= {1.0, 2.0} and (want["sigma"] > 0).any() and (want["sigma"] < 0).any()
        for k in ("h", "Wq"):
            assert k not in o or np.array_equal(R.r16(o[k], dtype), o[k])
        # the row before its 16-bit rounding, recomputed here: it must need none
        x = a * (want["z"] @ o["Wh"].T + o["bh"] + o["cls"][o["classes"]]) + o["pos"]
        assert np.array_equal(R.r16(x, dtype), x) and np.array_equal(want["dec"], x) and np.abs(x).max() >= 8
        # every partial sum in any order is a multiple of 1/4 below 2^22
        assert 4 * max(R.absdot(o["h"], o["Wl"]).max() + 2, a * (R.absdot(want["z"], o["Wh"]).max() + 2) + 2) < 2 ** 24
        assert (want["z"] != 0).mean() > 0.5 and (o["eps"] != 0).any()
    else:
        exact = R.BWD_EXACT + ("dlat",)
        for k in ("g", "dq", "Wt", "resid", "h"):
            assert np.array_equal(R.r16(o[k], dtype), o[k])
        if c.nq:
            v = o["dq"] @ o["Wt"].T + o["resid"]
            assert np.array_equal(R.r16(v, dtype), v) and np.array_equal(want["t"], a * v), "the proj form's t needs no rounding"
            assert 4 * (R.absdot(o["dq"], o["Wt"]).max() + 2) < 2 ** 24
        # dlat is a multiple of 1/4 (kl_weight gscale = 2, enc_scale eps a multiple of 1/4); the outer products' partial sums stay below 2^24
        assert np.array_equal(want["dlat"] * 4, np.round(want["dlat"] * 4))
        assert 4 * (np.abs(want["dlat"]).T @ np.abs(o["h"])).max() + 8 < 2 ** 24 and 4 * (np.abs(want["t"]).T @ np.abs(o["z"])).max() + 8 < 2 ** 24
        assert 4 * (np.abs(want["t"]) @ np.abs(o["Wh"])).max() < 2 ** 24
        assert set(np.unique(np.abs(o["sigma"]))) == {1.0, 2.0}
    assert all(fits32(want[k]) for k in exact)
    for order in ("seq", "pair"):
        got = R.run(c, o, dtype, prec=np.float32, order=order)
        for k in exact:
            assert np.array_equal(got[k], want[k]), (c.id, k, order)


# ------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.DT_NAME[d])
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_the_bounds_accept_an_fp32_evaluation_in_both_orders(c, dtype, mode):
    o = R.operands(c, dtype, mode)
    for order in ("seq", "pair"):
        verdict = R.judge(c, o, dtype, mode, R.run(c, o, dtype, prec=np.float32, order=order))
        for k, (bad, ratio, msg) in verdict.items():
            assert not bad, f"{order}: {msg}"
    if mode == "real":
        # a bound of the size of the result would accept anything
        for k, (ref, bound) in R.refs_of(c, o, dtype, R.run(c, o, dtype, prec=np.float32), mode).items():
            if k != "t16":
                assert np.median(bound) < 0.02 * max(np.median(np.abs(ref)), 1e-30), (c.id, k)


F, B = R.FWD, R.BWD
MUTANTS = [
    # (the wrong kernel, the cases it must be refused in, modes, the quantity that must leave its bound)
    ("drop_last@lat", F, ("pre-ragged", "z256", "de320"), R.MODES, "mu"),
    ("double_first@lat", F, ("pre-ragged", "z256", "de320"), R.MODES, "sigma"),
    ("drop_last@dec", F, ("pre-limits", "z260", "ragged"), R.MODES, "dec"),
    ("double_first@dec", F, ("pre-limits", "z260", "ragged"), R.MODES, "dec"),
    ("drop_last@qkv", F, ("proj64-nq200", "proj128-general", "proj256"), R.MODES, "qkv"),
    ("double_first@qkv", F, ("proj64-nq200", "proj128-general", "proj256"), R.MODES, "qkv"),
    ("drop_last@tproj", B, ("proj384", "proj768"), R.MODES, "t"),
    ("double_first@tproj", B, ("proj384", "proj768"), R.MODES, "t"),
    ("drop_last@dz", B, ("pre-limits", "four", "four-short"), R.MODES, "dlat"),
    ("double_first@dz", B, ("pre-limits", "four", "four-short"), R.MODES, "dlat"),
    ("drop_last@dh0", B, ("pre-ragged", "four", "scalar-two-rounds"), R.MODES, "denc"),
    ("double_first@dh0", B, ("pre-ragged", "four", "scalar-two-rounds"), R.MODES, "denc"),
    ("eps_next", F, ("pre-limits", "z256"), R.MODES, "z"),
    ("eps_next", B, ("pre-limits", "four"), R.MODES, "dlat"),
    ("kl_no_minus1", F, ("pre-limits", "z256"), R.MODES, "kl"),
    # (kl is exact in neither mode and its bound, a Z-term sum in any order, sits far above what the launches measure: one lost term
    # of the sum must still leave it, at every shape of the table)
    ("kl_drop_last", F, tuple(c.name for c in R.FWD), R.MODES, "kl"),
    ("s_plus_inv", B, ("pre-limits", "four", "scalar-de258"), R.MODES, "dlat"),
    ("no_gscale", B, ("pre-limits", "four", "scalar-de258"), R.MODES, "dlat"),
    ("no_enc_scale", B, ("pre-limits", "four", "scalar-de258"), R.MODES, "dlat"),
    ("t_unrounded", B, ("proj384", "proj768-resid"), ("real",), "t16"),   # (int mode: the value needs no rounding)
    ("cls_plus4", B, ("cls-b5", "cls-b64", "cls-b70"), R.MODES, "dcls"),
    ("pos_scaled", F, ("pre-limits", "z256", "proj256"), R.MODES, "dec"),
    ("outer_skip", B, ("pre-limits", "four", "cls-b70"), R.MODES, "dWl"),
]


@pytest.mark.parametrize("mut,table,names,modes,quantity", MUTANTS, ids=[f"{m[0]}-{'fwd' if m[1] is F else 'bwd'}" for m in MUTANTS])
def test_the_bounds_refuse_a_wrong_kernel(mut, table, names, modes, quantity):
    for name in names:
        c = by_name(table, name)
        for dtype in R.DTYPES:
            for mode in modes:
                o = R.operands(c, dtype, mode)
                verdict = R.judge(c, o, dtype, mode, R.run(c, o, dtype, prec=np.float32, mut=mut))
                assert verdict[quantity][0] > 0, f"{mut} passes as {quantity} of {c.id} ({R.DT_NAME[dtype]}, {mode})"
                if "@" in mut or mut in ("outer_skip", "pos_scaled", "kl_no_minus1"):
                    # a wrong sum is wrong in (nearly) every element, not in a lucky one
                    n = R.refs_of(c, o, dtype, R.run(c, o, dtype, prec=np.float32), mode)[quantity][0].size
                    assert verdict[quantity][0] >= 0.4 * n, (mut, c.id, mode, verdict[quantity][0], n)


# ------------------------------------------------------------------------------------------ the outer products on their own
def test_outer_jobs_cover_the_batch_sizes_and_types():
    jobs = [q for launch in R.OUTER for q in launch]
    assert {q.B for q in jobs} == {1, 3, 5, 33, 70} and {q.r for q in jobs} == {"f32", "bf16", "fp16"}
    assert {len(launch) for launch in R.OUTER} == {1, 2} and any(not q.bias for q in jobs)
    assert any(q.J * q.I % 64 for q in jobs) and all(q.r_pad for q in jobs if q.r != "f32" or q.B > 1)
    for mode in R.MODES:
        for launch, ops_ in zip(R.OUTER, R.outer_operands(mode)):
            for q, o in zip(launch, ops_):
                (ref, bound), bias = R.outer_refs(o["L"], o["R"], o["out0"], o["bias0"])
                for order in ("seq", "pair"):
                    out, ob = R.outer(o["L"], o["R"], o["out0"], o["bias0"], np.float32, order)
                    if mode == "int":
                        assert np.array_equal(out, ref) and (bias is None or np.array_equal(ob, bias[0]))
                    else:
                        assert (np.abs(out - ref) <= bound).all() and (bias is None or (np.abs(ob - bias[0]) <= bias[1]).all())
                wrong, _ = R.outer(o["L"], o["R"], o["out0"], o["bias0"], np.float32, mut="outer_skip")
                assert (np.abs(wrong - ref) > bound).mean() > (0.4 if mode == "int" else 0.9), (q, mode)
                assert np.array_equal(o["R"], R.f32(o["R"]) if q.r == "f32" else R.r16(o["R"], R.R_DTYPE[q.r]))
