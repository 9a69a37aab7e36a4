"""ctypes binding of libsdamd.so, read from the C ABI's own declaration (include/sd_amd.h) at import.

There is NO fallback: if the header or the shared library is missing or an entry point fails, this raises.  The
library is built in-tree by `__graft_entry__.build()` (hipcc --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsdamd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sd_amd.h")      # where csrc/sd_common.h includes it from

vp, i32, i64, f32, f64 = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double
SCALARS = {"int": i32, "long": i64, "float": f32, "double": f64}        # every other scalar C type is refused
_DECL = re.compile(r"\s*(?:(.*\*)\s*(\w+)|(\w[\w\s]*?)\s+(\w+))\s*", re.S)           # "const T* p" | "type name"
_ARGS_BLOCK = re.compile(r"const (sda_\w+_args)\*")
_STRUCT_NAMES = {"sda_conv_args": "ConvArgs", "sda_wgrad_args": "WgradArgs", "sda_pack_desc": "PackDesc",
                 "sda_pgemm_args": "PgemmArgs", "sda_adam_desc": "AdamDesc"}


class SdaError(RuntimeError):
    pass


def parse_header(text):
    """The C ABI as sd_amd.h declares it -> (constants, structs, signatures, prototypes):
    {name without SDA_: int}, {sda_x: ctypes.Structure, fields in header order}, {sda_f: (restype, argtypes)} and, for the tests
    to lay against the C compiler, {sda_f: (C return type, [C argument types])}.  It reads the C this header uses and nothing
    more: whatever it cannot read it refuses with an SdaError that names the declaration."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#define[ \t]+SDA_(\w+)[ \t]+(\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S), flags=re.M)
    structs, sigs, protos = {}, {}, {}

    def split(decl, where):                 # "const float* x" -> ("const float*", "x")
        m = _DECL.fullmatch(decl)
        if not m:
            raise SdaError(f"sd_amd.h, {where}: cannot read '{decl.strip()}'")
        return " ".join((m[1] or m[3]).split()).replace(" *", "*"), m[2] or m[4]

    def scalar(c, where):
        if c not in SCALARS:
            raise SdaError(f"sd_amd.h, {where}: no ctypes type for '{c}'")
        return SCALARS[c]

    def ctype(c, where):                    # a host argument block (const sda_*_args*) by reference, any other pointer as void*
        if not c.endswith("*"):
            return scalar(c, where)
        m = _ARGS_BLOCK.fullmatch(c)
        if m and m[1] not in structs:
            raise SdaError(f"sd_amd.h, {where}: '{c}' before the struct's declaration")
        return C.POINTER(structs[m[1]]) if m else vp

    def enum(m):
        for item in m[1].split(","):
            e = re.fullmatch(r"\s*SDA_(\w+)\s*=\s*(\d+)\s*", item)
            if not e:
                raise SdaError(f"sd_amd.h: cannot read the enumerator '{item.strip()}'")
            consts[e[1]] = int(e[2])
        return " "

    def struct(m):
        fields = []
        for stmt in filter(None, (s.strip() for s in m[2].split(";"))):         # "type a, b, c" or "const T* p"
            first, *more = stmt.split(",")
            c, name = split(first, m[1])
            if more and (c.endswith("*") or not all(re.fullmatch(r"\s*\w+\s*", n) for n in more)) or m[3] != m[1]:
                raise SdaError(f"sd_amd.h, {m[1]}: cannot split '{stmt}'")
            fields += [(n.strip(), ctype(c, m[1])) for n in [name, *more]]
        structs[m[1]] = type(_STRUCT_NAMES.get(m[1], m[1]), (C.Structure,), {"_fields_": fields})
        return " "

    def prototype(m):
        ret, name = " ".join(m[1].split()).replace(" *", "*"), m[2]
        args = [] if m[3].strip() == "void" else [split(a, name)[0] for a in m[3].split(",")]
        protos[name] = (ret, args)
        sigs[name] = (C.c_char_p if ret == "const char*" else scalar(ret, name), [ctype(a, name) for a in args])
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(sda_\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"([\w\s*]+?)\b(sda_\w+)\s*\(([^()]*)\)\s*;", prototype, text)
    if text.strip():                        # everything was read, or it is refused: nothing is skipped
        m = re.search(r"sda_\w+", text)
        raise SdaError(f"sd_amd.h: cannot read the declaration of '{m[0] if m else text.strip()[:60]}'")
    return consts, structs, sigs, protos


def read_abi(path=HEADER_PATH):
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise SdaError(f"{path}: the C ABI's declaration is needed to bind libsdamd.so ({e})") from None


# SIGNATURES: name -> (restype, argtypes) of every symbol sd_amd.h declares; the constants under their header names without
# SDA_ (ABI_VERSION, ROW_PAD, CH_ALIGN, F32 / BF16 / F16, EPI_*, CONV_*, WGRAD_FLAT_ROWS, MSE_PARTIALS, ...)
CONSTANTS, STRUCTS, SIGNATURES, PROTOTYPES = read_abi()
globals().update(CONSTANTS)
ConvArgs, WgradArgs, PackDesc, PgemmArgs, AdamDesc = (STRUCTS[n] for n in _STRUCT_NAMES)

_lib = None


def load():
    """Load libsdamd.so and bind every declared symbol; raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdaError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C speech_decoding_amd/csrc`.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.sda_abi_version() != ABI_VERSION:
        raise SdaError("libsdamd.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().sda_last_error()
        raise SdaError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def pad_channels(c: int) -> int:
    return (c + CH_ALIGN - 1) // CH_ALIGN * CH_ALIGN


def rows_tp(T: int) -> int:
    return T + ROW_PAD


def rows_alloc(B: int, T: int) -> int:
    return B * rows_tp(T) + ROW_PAD + 128 + 2 * ROW_PAD
