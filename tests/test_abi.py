"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/mst_hip.h declares (no kernel is launched here)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from musicstyletransfer_amd.csrc import build
    build.build(verbose=False)
    from musicstyletransfer_amd import _lib
    return _lib.load()


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mst_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mst_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/mst_hip.h but not exported"


REMOVED = ["mst_gemm_wgrad", "mst_gemm_wgrad_batch", "mst_gemm_wgrad_batch_ws", "mst_gemm_wgrad_batch_sums", "mst_step_begin_v",
           "mst_device_count", "mst_adam_flat_emb", "mst_adam_flat_sched", "mst_adam_flat_emb_sched", "mst_adam_flat_gnorm",
           "mst_adam_flat_ema"]


def test_exports_are_exactly_the_declarations(lib):
    """the dynamic symbol table of the built library, read by a binutils-style nm: nothing declared is missing, nothing
    exported is undeclared (diagnostic builds' mst_debug_* aside), and the forwarding entry points ABI 101 dropped are gone"""
    import shutil, subprocess
    from musicstyletransfer_amd import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("mst_")}
    exported = {s for s in exported if not s.startswith("mst_debug_")}
    assert exported == set(declared_symbols()) == set(_lib.SIGNATURES)
    for name in REMOVED:
        assert name not in exported and name not in _lib.SIGNATURES


def test_version_and_error_string(lib):
    assert lib.mst_version() >= 121  # 121: mst_layernorm_form, mst_group_colsum_form
    assert isinstance(lib.mst_last_error(), bytes)


def test_struct_layouts_match_c(lib):
    """sizeof of every struct, offsetof and size of every field, from gcc reading the real header (so independent of the
    binding's parser, which only supplies the names to ask about)"""
    import ctypes, subprocess, tempfile
    from musicstyletransfer_amd import _lib
    assert len(_lib.STRUCTS) == 12
    lines = []
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mst_hip.h"\nint main(){\n' + "\n".join(lines) + "\nreturn 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = iter(subprocess.check_output([exe], text=True).splitlines())
    n_fields = 0
    for cname, cls in _lib.STRUCTS.items():
        assert ctypes.sizeof(cls) == int(next(got)), cname
        for f, _ in cls._fields_:
            off, size = map(int, next(got).split())
            assert (getattr(cls, f).offset, getattr(cls, f).size) == (off, size), f"{cname}.{f}"
            n_fields += 1
    assert n_fields >= 240 and next(got, None) is None
    # Python names the package, the tests and tools/ use
    for py in ("GemmArgs BceArgs RowTailArgs RowTailBwdArgs LnArgs LnBwdIn StepMetrics PartialSum StepBeginArgs OuterJob "
               "WgradArgs AdamArgs").split():
        assert getattr(_lib, py) in _lib.STRUCTS.values()


def test_parser_known_answers():
    """argument lists written out by hand (they are the hand-written table's, from before the binding read the header)"""
    import ctypes as C
    from musicstyletransfer_amd import _lib
    i32, i64, f32, f64, u64, u32, vp, ci = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int
    P = C.POINTER
    want = {
        "mst_version": (ci, []),
        "mst_last_error": (C.c_char_p, []),
        "mst_graph_end": (ci, [vp, P(vp)]),
        "mst_gemm_nt_ln_parts": (i64, [i64]),
        "mst_layernorm_bwd_parts": (i64, [i64, i64]),
        "mst_layernorm_form": (ci, [ci, ci, i64, i64, vp]),
        "mst_group_colsum_form": (ci, [i64, i64, vp]),
        "mst_adam_flat": (ci, [P(_lib.AdamArgs), vp]),
        "mst_adam_flat_form": (ci, [P(_lib.AdamArgs), vp]),
        "mst_latent_rows": (ci, [ci, i64, i64, i64, i64, vp, vp, vp, vp, vp, ci, f32, u64, vp, u32, i64, vp, vp,
                                 vp, vp, vp, vp, i64, i64, vp, f32, vp, vp, i64, vp]),
        "mst_attn_decode": (ci, [ci, i64, i64, i64, i64, i64, vp, i64, i64, i64, i64, ci, vp, i64, vp]),
        "mst_row_tail_fwd_ride_shadows": (ci, [P(_lib.RowTailArgs), P(_lib.GemmArgs), vp, ci, vp, vp, vp, vp, i64, i64, vp]),
        "mst_layernorm_bwd": (ci, [ci, i64, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64,
                                   vp, i64, vp, vp, ci, f32, u64, u32, vp, i64, vp, vp]),
        "mst_gemm_wgrad_batch_flush": (ci, [P(_lib.WgradArgs), ci, vp, i64, P(_lib.PartialSum), ci, P(_lib.OuterJob), ci, vp]),
        "mst_gemm_wgrad_plan": (ci, [P(_lib.WgradArgs), ci, i64, vp]),
        "mst_attn_fwd_form": (ci, [ci, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, ci, i64, i64, vp]),
        "mst_attn_bwd_form": (ci, [ci, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, vp]),
        "mst_latent_form": (ci, [i64, i64, i64, i64, vp, vp]),
        "mst_row_tail_form": (ci, [ci, ci, i64, P(_lib.GemmArgs), i64, vp]),
        "mst_sigmoid_bce": (ci, [ci, i64, i64, i64, vp, i64, vp, f32, ci, vp, vp, vp, i64, vp, i64, f32, ci, vp]),
        "mst_sigmoid_bce_form": (ci, [ci, i64, i64, i64, vp, i64, vp, f32, ci, vp, vp, vp, i64, vp, i64, f32, ci, vp]),
        "mst_gemm_sigmoid_bce": (ci, [P(_lib.GemmArgs), P(_lib.BceArgs), vp]),
        "mst_gemm_sigmoid_bce_form": (ci, [P(_lib.GemmArgs), P(_lib.BceArgs), P(_lib.GemmArgs), P(_lib.LnArgs), vp]),
        "mst_step_begin": (ci, [P(_lib.StepBeginArgs), vp]),
        "mst_mask_from_lengths": (ci, [i64, i64, vp, i32, vp, vp]),
    }
    assert len(want["mst_latent_rows"][1]) == 30
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
    assert _lib.StepMetrics._fields_ == [
        ("B", i64), ("recon", vp), ("kl", vp), ("kl_weight", f32), ("total", vp), ("metric", vp),
        ("status", vp), ("expect_ptr0", vp), ("expect_val0", u32), ("expect_ptr1", vp), ("expect_val1", u32),
        ("fin_recon", vp), ("fin_kl", vp), ("fin_B", i64)]
    assert (_lib.MST_BF16, _lib.MST_F16, _lib.MST_F32, _lib.ACT_NONE, _lib.ACT_RELU) == (0, 1, 2, 0, 1)
    assert (_lib.CE_MAX_WORKGROUPS, _lib.TAIL_SPIN_FWD, _lib.TAIL_SPIN_BWD, _lib.STEP_INCOMPLETE) == (4096, 1, 2, 16)


GOOD_STRUCT = "typedef struct mst_ln_args { int32_t mode; /* c */ const float* gamma; int64_t a, b; } mst_ln_args;\n"


def test_parser_reads_the_headers_style():
    import ctypes as C
    from musicstyletransfer_amd import _lib
    structs, sigs, consts = _lib.parse_header(
        "#ifndef G\n#define G\n#include <stdint.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\ntypedef void* mst_stream_t; // s\n"
        "enum mst_e { MST_A = 0, MST_B = -3 };\n#define MST_N 7u /* n */\n" + GOOD_STRUCT +
        "int mst_f(const mst_ln_args* a, int n /* , int m */,\n  double x, mst_stream_t s); int64_t mst_g(void);\n"
        "#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert [(n, t) for n, t in structs["mst_ln_args"]._fields_] == [("mode", C.c_int32), ("gamma", C.c_void_p), ("a", C.c_int64),
                                                                    ("b", C.c_int64)]
    assert sigs == {"mst_f": (C.c_int, [C.POINTER(structs["mst_ln_args"]), C.c_int, C.c_double, C.c_void_p]), "mst_g": (C.c_int64, [])}
    assert consts == {"MST_A": 0, "MST_B": -3, "MST_N": 7}


@pytest.mark.parametrize("what, text", [
    ("unknown type name", "int mst_f(size_t n);"),
    ("unknown type name behind a pointer", "int mst_f(const half* x);"),
    ("two-word type", "int mst_f(unsigned int n);"),
    ("unknown field type", "typedef struct mst_ln_args { long n; } mst_ln_args;"),
    ("array field", "typedef struct mst_ln_args { int32_t n[4]; } mst_ln_args;"),
    ("function pointer field", "typedef struct mst_ln_args { int (*f)(int); } mst_ln_args;"),
    ("function pointer parameter", "int mst_f(int (*cb)(int), int n);"),
    ("bit-field", "typedef struct mst_ln_args { int32_t n : 3; } mst_ln_args;"),
    ("star on a second declarator", "typedef struct mst_ln_args { int64_t a, *b; } mst_ln_args;"),
    ("star with several declarators", "typedef struct mst_ln_args { int64_t *a, b; } mst_ln_args;"),
    ("prototype that cannot be split", "int mst_f(int a, int b) __attribute__((cold));"),
    ("prototype without a return type", "mst_f(int a);"),
    ("unnamed parameter", "int mst_f(int, int b);"),
    ("struct used before its declaration", "int mst_f(const mst_ln_args* a);\n" + GOOD_STRUCT),
    ("struct by value", GOOD_STRUCT + "int mst_f(mst_ln_args a);"),
    ("struct without a Python name", "typedef struct mst_new_args { int32_t n; } mst_new_args;"),
    ("struct declared twice", GOOD_STRUCT + GOOD_STRUCT),
    ("pointer to pointer other than void**", "int mst_f(float** x);"),
    ("char* parameter", "int mst_f(const char* name);"),
    ("enumerator without a value", "enum mst_e { MST_A, MST_B };"),
    ("#define that is not an integer", "#define MST_X (1 << 4)"),
    ("nested braces", "typedef struct mst_ln_args { struct { int32_t n; } in; } mst_ln_args;"),
    ("unterminated declaration", "int mst_f(int a)"),
])
def test_parser_refuses(what, text):
    from musicstyletransfer_amd import _lib
    with pytest.raises(_lib.MstError, match="mst_hip.h"):
        _lib.parse_header("typedef void* mst_stream_t;\n" + text)


def test_invalid_arguments_fail_loudly(lib):
    # argument validation happens before any HIP call, so it is testable without a GPU
    import ctypes
    from musicstyletransfer_amd import _lib
    g = _lib.GemmArgs()
    g.M, g.N, g.K = 4, 4, 3  # K not a multiple of 8
    rc = lib.mst_gemm_nt(ctypes.byref(g), None)
    assert rc == -1
    assert b"multiples of 8" in lib.mst_last_error()
    with pytest.raises(_lib.MstError):
        _lib.call("mst_layernorm_fwd", 0, 4, 6, None, 8, None, None, 1e-5, None, 8, None, None, 1, None)
