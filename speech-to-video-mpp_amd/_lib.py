"""ctypes binding of libs2v.so, derived from the C ABI's own declaration (include/s2v.h).

The header is parsed once at import: its enumerators and ``#define`` become this module's constants
(``S2V_ACT_RELU`` -> ``ACT_RELU``), ``s2v_conv_params`` becomes ``ConvParams`` and every prototype an
entry of ``_SIGS``, so a new entry point needs no edit here.  The parser knows exactly what the header
uses and raises on anything else.

The library is built in-tree (``make -C speech-to-video-mpp_amd/csrc`` or
``__graft_entry__.build()``) and loaded from this package directory only.  There is no CPU
fallback anywhere on the product path: if the library is missing, every op raises.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
# the package's in-tree build (libs2v_torch.so, the model path's launch ops, links this same file)
LIB_PATH = os.path.join(_PKG, "libs2v.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "s2v.h")


class S2VError(RuntimeError):
    pass


class ConvParams(ctypes.Structure):
    """s2v_conv_params; its ``_fields_`` are the header's members, set below."""


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long": ctypes.c_long,
            "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "s2v_stream_t": ctypes.c_void_p}


def _decl(text, base=None):
    """One declarator, ``const float *x`` -> ("float", True, "x").  ``base``: the type that a later
    declarator of a member list (``int n, h;``) inherits; it may then only add ``*``."""
    tok = re.findall(r"\w+|\S", text)
    if not tok or tok[-1] == "const" or not all(re.fullmatch(r"\w+|\*", t) for t in tok):
        raise S2VError(f"s2v.h: cannot parse the declaration {text.strip()!r}")
    name = tok.pop()
    stars = tok.index("*") if "*" in tok else len(tok)
    words = [t for t in tok[:stars] if t != "const"]
    if set(tok[stars:]) - {"*", "const"} or (base is not None and words):
        raise S2VError(f"s2v.h: cannot parse the declaration {text.strip()!r}")
    return (" ".join(words) if base is None else base), stars < len(tok), name


def _ctype(base, pointer, text, ret=False):
    """The ctypes type of a parameter or struct member (``ret``: of a return value); ``text`` is for the error."""
    if pointer and ret and base == "char":
        return ctypes.c_char_p
    if pointer and not ret:
        return ctypes.POINTER(ConvParams) if base == "s2v_conv_params" else ctypes.c_void_p
    if pointer or base not in _SCALARS:
        raise S2VError(f"s2v.h: unknown type {base + ' *' * pointer!r} in {text.strip()!r}")
    return _SCALARS[base]


def parse_header(text):
    """The C declarations of ``text`` -> (consts, structs, sigs): name -> int, struct name -> [(member, ctype)],
    function name -> (restype, argtypes).  Raises S2VError, naming the text, on whatever it does not know."""
    consts, structs, sigs = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#\s*ifdef\s+__cplusplus\b.*?^[ \t]*#\s*endif\b", "", text, flags=re.S | re.M)
    for line in re.findall(r"^[ \t]*#\s*define[ \t]+(.*?)[ \t]*$", text, flags=re.M):
        name, *value = line.split(None, 1)
        if value and not re.fullmatch(r"-?\d+", value[0]):
            raise S2VError(f"s2v.h: #define {line!r} is not an integer")
        if value:                                            # (the include guard defines no value)
            consts[name] = int(value[0])
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    pos, stmt = 0, re.compile(r"\s*((?:[^;{}]|\{[^{}]*\})*);")
    while m := stmt.match(text, pos):
        pos, s = m.end(), " ".join(m[1].split())
        if e := re.fullmatch(r"enum \{(.*)\}", s):
            for item in filter(None, map(str.strip, e[1].split(","))):
                if not (v := re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)):
                    raise S2VError(f"s2v.h: enumerator {item!r} has no explicit integer value")
                consts[v[1]] = int(v[2])
        elif t := re.fullmatch(r"typedef struct (\w+) \{(.*)\} \1", s):
            fields = structs[t[1]] = []
            for member in filter(None, map(str.strip, t[2].split(";"))):
                base = None
                for d in member.split(","):
                    base, pointer, name = _decl(d, base)
                    fields.append((name, _ctype(base, pointer, member)))
        elif f := re.fullmatch(r"(.*\bs2v_\w+) ?\((.*)\)", s):
            base, pointer, name = _decl(f[1])
            args = [] if f[2].strip() == "void" else [_decl(a)[:2] + (a,) for a in f[2].split(",")]
            sigs[name] = (_ctype(base, pointer, s, ret=True), [_ctype(*a) for a in args])
        elif s != "typedef void *s2v_stream_t":
            raise S2VError(f"s2v.h: cannot parse the declaration {s!r}")
    if text[pos:].strip():
        raise S2VError(f"s2v.h: cannot parse the declaration {text[pos:].strip()[:80]!r}")
    return consts, structs, sigs


def _read_header(path):
    if not os.path.exists(path):
        raise S2VError(f"{path} is missing: the ctypes binding of libs2v.so is derived from it "
                       "(the package runs from its source tree, beside include/)")
    with open(path) as f:
        return f.read()


_consts, _structs, _SIGS = parse_header(_read_header(HEADER_PATH))      # _SIGS: name -> (restype, argtypes)
ConvParams._fields_ = _structs["s2v_conv_params"]
globals().update({k.removeprefix("S2V_"): v for k, v in _consts.items()})    # ACT_*, IN_*, PREC_*, TUNE_*, ...

EXPORTS = tuple(_SIGS)

_lock = threading.Lock()
_lib = None


def load():
    """Load libs2v.so (raises if it was not built — there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise S2VError(f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}/csrc` "
                               "(or __graft_entry__.build()); the HIP path has no CPU fallback")
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().s2v_last_error().decode(errors="replace")
        raise S2VError(f"{what} failed ({rc}): {msg}")
