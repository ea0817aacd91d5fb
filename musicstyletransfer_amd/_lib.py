"""ctypes binding of libmst_hip.so (include/mst_hip.h).

The product path has NO CPU fallback: if the shared object is missing, or a kernel returns a
non-zero status, an exception is raised. `load()` only dlopen()s and checks the exported symbols
(so it works on a GPU-less box for the "does it build / export" tests); anything that launches a
kernel needs a visible HIP device.
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libmst_hip.so")

HEADER_PATH = os.path.join(HERE, "..", "include", "mst_hip.h")


class MstError(RuntimeError):
    pass


c_i32, c_i64, c_f32, c_f64, c_u64, c_u32 = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_uint64, C.c_uint32
_SCALARS = {"int": C.c_int, "int32_t": c_i32, "int64_t": c_i64, "uint8_t": C.c_uint8, "uint32_t": c_u32, "uint64_t": c_u64,
            "float": c_f32, "double": c_f64, "mst_stream_t": C.c_void_p}
# Python class of every struct the header declares (a new struct needs a name here)
_STRUCT_NAMES = {"mst_gemm_args": "GemmArgs", "mst_bce_args": "BceArgs", "mst_row_tail_args": "RowTailArgs",
                 "mst_row_tail_bwd_args": "RowTailBwdArgs", "mst_ln_args": "LnArgs", "mst_ln_bwd_in": "LnBwdIn",
                 "mst_step_metrics": "StepMetrics", "mst_partial_sum": "PartialSum", "mst_step_begin_args": "StepBeginArgs",
                 "mst_outer_job": "OuterJob", "mst_wgrad_args": "WgradArgs", "mst_adam_args": "AdamArgs"}

# one top-level declaration: a struct typedef, an enum, the stream typedef, or (anything else up to its ';') a prototype
_DECL = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;|enum\s+\w+\s*\{([^{}]*)\}\s*;"
                   r"|typedef\s+void\s*\*\s*mst_stream_t\s*;|([^;{}]+);)")
_FIELD = re.compile(r"(?:const\s+)?(\w+)\b\s*(\*?)\s*(\w+)((?:\s*,\s*\w+)*)$")  # `type a, b` or `const type* a`
_PARAM = re.compile(r"(?:const\s+)?(\w+)\b\s*(\*{0,2})\s*\w+$")
_PROTO = re.compile(r"(?:const\s+)?(\w+)\b\s*(\*?)\s*(mst_\w+)\s*\(([^()]*)\)$")


def parse_header(text):
    """The C ABI as include/mst_hip.h states it, in the header's own style and no more: ({struct name: ctypes.Structure class},
    {function: (restype, argtypes)}, {enumerator or #define: int}). Whatever is not understood raises MstError."""
    structs, signatures, constants = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S)  # extern "C" { and its }
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(.*)$", text, flags=re.M):
        m = re.match(r"(\w+)(?:\s+(\d+)[uU]?)?\s*$", line)
        if not m:
            raise MstError(f"mst_hip.h: cannot read `#define {line.strip()}`")
        if m.group(2):  # (a bare name is the include guard)
            constants[m.group(1)] = int(m.group(2))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def ctype(base, stars, decl, ret=False):
        if base not in _SCALARS and base not in structs and not (stars and base in ("void", "char")):
            raise MstError(f"mst_hip.h: unknown type `{base}` in `{decl}`")
        if base == "char" and not ret:
            raise MstError(f"mst_hip.h: `char*` is bound as a return type only: `{decl}`")
        if stars == "**" and base != "void":
            raise MstError(f"mst_hip.h: `{base}**` in `{decl}`")
        if not stars:
            if base in structs:
                raise MstError(f"mst_hip.h: struct by value in `{decl}`")
            return _SCALARS[base]
        return (C.POINTER(C.c_void_p) if stars == "**" else C.POINTER(structs[base]) if base in structs
                else C.c_char_p if base == "char" else C.c_void_p)

    pos = 0
    while text[pos:].strip():
        m = _DECL.match(text, pos)
        if not m:
            raise MstError(f"mst_hip.h: cannot read the declaration at `{' '.join(text[pos:pos + 80].split())}`")
        pos = m.end()
        tag, body, name, enum_body, proto = m.groups()
        if tag is not None:
            if tag != name or name in structs or name not in _STRUCT_NAMES:
                raise MstError(f"mst_hip.h: struct `{tag}` / `{name}`: mismatching, repeated or without a Python name")
            fields = []
            for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
                f = _FIELD.match(decl)
                if not f or (f.group(2) and f.group(4)):
                    raise MstError(f"mst_hip.h: cannot read field `{decl}` of {name}")
                t = ctype(f.group(1), f.group(2), decl)
                fields += [(n.strip(), t) for n in (f.group(3) + f.group(4)).split(",")]
            structs[name] = type(_STRUCT_NAMES[name], (C.Structure,), {"_fields_": fields})
        elif enum_body is not None:
            for item in filter(None, (e.strip() for e in enum_body.split(","))):
                e = re.match(r"(\w+)\s*=\s*(-?\d+)$", item)
                if not e:
                    raise MstError(f"mst_hip.h: cannot read enumerator `{item}`")
                constants[e.group(1)] = int(e.group(2))
        elif proto is not None:
            decl = " ".join(proto.split())
            f = _PROTO.match(decl)
            if not f:
                raise MstError(f"mst_hip.h: cannot read prototype `{decl}`")
            args = []
            for prm in ([] if f.group(4).strip() == "void" else f.group(4).split(",")):
                a = _PARAM.match(prm.strip())
                if not a:
                    raise MstError(f"mst_hip.h: cannot read parameter `{prm.strip()}` of {f.group(3)}")
                args.append(ctype(a.group(1), a.group(2), decl))
            signatures[f.group(3)] = (ctype(f.group(1), f.group(2), decl, ret=True), args)
    return structs, signatures, constants


try:
    with open(HEADER_PATH) as _f:
        STRUCTS, SIGNATURES, _consts = parse_header(_f.read())
except OSError as e:
    raise MstError(f"{HEADER_PATH} is missing: the binding is read from it") from e
globals().update({cls.__name__: cls for cls in STRUCTS.values()})  # GemmArgs, LnArgs, ... (_STRUCT_NAMES)
MST_BF16, MST_F16, MST_F32 = _consts["MST_BF16"], _consts["MST_F16"], _consts["MST_F32"]
ACT_NONE, ACT_RELU = _consts["MST_ACT_NONE"], _consts["MST_ACT_RELU"]
CE_MAX_WORKGROUPS = _consts["MST_CE_MAX_WORKGROUPS"]  # rows of mst_softmax_ce's token-metric partials
ROLL_SLOTS = _consts["MST_ROLL_SLOTS"]  # slots of the BCE launches' piano-roll counts
# flags of the sticky step-status word
TAIL_SPIN_FWD, TAIL_SPIN_BWD, STEP_INCOMPLETE = (_consts[k] for k in ("MST_TAIL_SPIN_FWD", "MST_TAIL_SPIN_BWD", "MST_STEP_INCOMPLETE"))

_lib = None


def load():
    """dlopen libmst_hip.so and bind every declared symbol. Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MstError(
            f"{LIB_PATH} is missing: build it with `python -m musicstyletransfer_amd.csrc.build` "
            "(there is no CPU fallback for the training step)")
    # PyTorch-ROCm wheels bundle their own libamdhip64.so.7. It must be in the process BEFORE this library
    # is dlopen()ed, so that our NEEDED libamdhip64.so.7 binds to that same runtime instance (same SONAME):
    # torch's hipStream_t handles and device pointers are then valid in our launches. Loaded the other way
    # round, two HIP runtimes coexist and the second reports "no ROCm-capable device".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise MstError(f"libmst_hip.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().mst_last_error()
        raise MstError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    check(rc, name)
