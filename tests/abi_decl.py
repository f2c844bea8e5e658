"""The one reader of the C headers under include/ that the tests share: declared names, parsed declarations, struct fields, constants,
and the rule by which a C type corresponds to a ctypes type.  tests/test_abi_host.py holds ampligraph_amd/_ffi.py equal to the headers
with it; the guard-band tests ask it which entry points a header declares."""
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
STRUCTS = {"amdkge_model": "Model", "amdkge_loss": "Loss", "amdkge_opt": "Opt", "amdkge_session_config": "SessionConfig"}   # -> _ffi's Structure
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
POINTEES = dict(SCALARS, uint8_t=C.c_uint8, uint32_t=C.c_uint32)
HEADERS = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))


def text(header, comments=True):
    with open(os.path.join(INCLUDE, header)) as f:
        return f.read() if comments else re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def declared_names(header):
    """Every amdkge_* name followed by a parenthesis in the RAW text, comments included (the loose form: it also sees an entry point a
    comment writes as a call).  What the "frozen header" and "every entry point has a case" assertions compare."""
    return set(re.findall(r"\b(amdkge_[a-z0-9_]+)\s*\(", text(header)))


def _param(p):
    """'const float* d_ent' -> ('const float*', 'd_ent'): the stars belong to the type, whichever side they were written on"""
    m = re.fullmatch(r"(.*?)(\w+)", " ".join(p.split()))
    return re.sub(r"\s*\*", "*", m.group(1)).strip(), m.group(2)


def declarations(header):
    """{name: (restype text, [(C type text, parameter name), ...])} of the function declarations, comments stripped"""
    found = re.findall(r"^[ \t]*(const char\*|int64_t|int32_t|int|void)\s+(amdkge_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", text(header, False), flags=re.M)
    assert len({name for _, name, _ in found}) == len(found)
    return {name: (res, [] if params.strip() == "void" else [_param(p) for p in params.split(",")]) for res, name, params in found}


def struct_fields(header):
    """{struct: [(C type text, field name), ...]} of the `typedef struct NAME { ... } NAME;` definitions (`float beta1, beta2;` is two)"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text(header, False), flags=re.S):
        out[name] = []
        for first, *more in (d.split(",") for d in body.split(";") if d.strip()):
            ctype, field = _param(first)
            out[name] += [(ctype, field)] + [(ctype, m.strip()) for m in more]
    return out


def constant_names(header):
    """every enum member and every object-like `#define AMDKGE_* value` (an include guard has no value)"""
    src = text(header, False)
    names = [part.split("=")[0].strip() for body in re.findall(r"\benum\s*\{(.*?)\}", src, flags=re.S) for part in body.split(",") if part.strip()]
    names += re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AMDKGE_[A-Z0-9_]+)[ \t]+\S", src, flags=re.M)
    assert all(re.fullmatch(r"AMDKGE_[A-Z0-9_]+", n) for n in names), names
    return names


def matches(c_type, ct, ffi):
    """Does the ctypes type `ct` stand for the C return, parameter or field type `c_type`?  A scalar: exactly its ctypes type.  One of
    STRUCTS: POINTER of that Structure (by value: the Structure).  T**: POINTER(c_void_p).  Any other pointer: c_void_p, or POINTER(T')
    whose pointee matches T.  The return types void: None, and const char*: c_char_p."""
    t = re.sub(r"\bconst\b", " ", c_type).strip()
    base = t.rstrip("*").strip()
    if t in ("void", "char*"):
        return ct is (None if t == "void" else C.c_char_p)
    if t.endswith("**"):
        return ct == C.POINTER(C.c_void_p)
    if base in STRUCTS:
        return ct == (C.POINTER(getattr(ffi, STRUCTS[base])) if t.endswith("*") else getattr(ffi, STRUCTS[base]))
    if t.endswith("*"):
        return ct is C.c_void_p or (base in POINTEES and ct == C.POINTER(POINTEES[base]))
    return ct is SCALARS[t]
