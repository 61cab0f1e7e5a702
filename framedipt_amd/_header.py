"""Reader of ``include/fdipt.h``: the structs, prototypes and integer macros of the C ABI as ctypes objects.

The header keeps to one declaration style (stated in its top comment) and this reader understands that style only.  Whatever else it
meets - an unknown type, an unnamed parameter, a function pointer, a bit-field, an array member, a struct by value, an ``FDIPT_`` macro
that is no integer - raises ``HeaderError`` with the declaration quoted: a binding that guessed would corrupt arguments silently.
"""
from __future__ import annotations

import collections
import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong}
_POINTEES = set(SCALARS) | {"void", "char", "uint8_t"}  # what a plain (void*) pointer may point to, beside the header's own structs
_DECL = re.compile(r"(?:const )?(unsigned long long|\w+)(\**) (\w+(?: ?, ?\w+)*)")  # [const] type[*[*]] name[, name ...]
_INTEGER = re.compile(r"\d+|\( ?-?\d+ ?\)")

# structs: C name -> ctypes.Structure subclass (named without the Fdipt prefix), functions: name -> (restype, argtypes, parameter names),
# macros: name without the FDIPT_ prefix -> int
Header = collections.namedtuple("Header", "structs functions macros")


class HeaderError(ValueError):
    pass


def _ctype(base, stars, name, structs, parameter):
    """The ctypes type of one declarator, or None where the rules do not cover it."""
    if not stars:
        return C.c_void_p if base == "fdipt_stream_t" else SCALARS.get(base)
    if stars != "*":
        return C.POINTER(C.c_void_p) if (base, stars) == ("void", "**") else None
    if parameter and base in structs:
        return C.POINTER(structs[base])
    if parameter and base in SCALARS and name.endswith("_host"):
        return C.POINTER(SCALARS[base])
    return C.c_void_p if base in _POINTEES or base in structs else None


def _declaration(text, structs, parameter, where):
    """``text`` ("const float* x", "int32_t B, N") as a list of (name, ctype)."""
    m = _DECL.fullmatch(text)
    names = re.split(" ?, ?", m.group(3)) if m else []
    if len(names) > 1 and (parameter or m.group(2)):  # several names share a scalar type in a struct only
        names = []
    types = [_ctype(m.group(1), m.group(2), n, structs, parameter) for n in names]
    if not types or None in types:
        raise HeaderError(f"fdipt.h: cannot read the declaration '{text}' in '{where}'")
    return list(zip(names, types))


def parse(text):
    """Structs, prototypes and integer macros of the header ``text`` as a ``Header``."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    guard = re.search(r"^#ifndef (\w+)", text, re.M)
    macros = {}
    for name, body in re.findall(r"^#[ \t]*define[ \t]+(\w+)(.*)$", text, re.M):
        body = body.strip()
        if _INTEGER.fullmatch(body) and name.startswith("FDIPT_"):
            macros[name[len("FDIPT_"):]] = int(body.strip("() "))
        elif name.startswith("FDIPT_") and not (guard and name == guard.group(1) and not body):
            raise HeaderError(f"fdipt.h: the macro '#define {name} {body}' is not an integer")
    text = " ".join(re.sub(r"^#.*$", " ", text, flags=re.M).split())

    structs = {}

    def struct(m):
        tag, body, name = m.groups()
        if tag != name or not name.startswith("Fdipt"):
            raise HeaderError(f"fdipt.h: cannot read 'typedef struct {tag} {{...}} {name};'")
        fields = [f for d in body.split(";") if d.strip() for f in _declaration(d.strip(), structs, False, "struct " + name)]
        structs[name] = type(name[len("Fdipt"):], (C.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"typedef struct (\w+) ?\{(.*?)\} ?(\w+) ?;", struct, text)
    functions = {}
    for statement in (s.strip() for s in text.split(";")):
        if not statement or statement == "typedef void* fdipt_stream_t":
            continue
        m = re.fullmatch(r"(const char\*|\w+) (fdipt_\w+) ?\((.*)\)", statement)
        restype = m and (C.c_char_p if m.group(1) == "const char*" else SCALARS.get(m.group(1)))
        if not restype:
            raise HeaderError(f"fdipt.h: cannot read the declaration '{statement}'")
        parameters = [] if m.group(3).strip() == "void" else [
            _declaration(p.strip(), structs, True, statement)[0] for p in m.group(3).split(",")]
        functions[m.group(2)] = (restype, [t for _, t in parameters], [n for n, _ in parameters])
    return Header(structs, functions, macros)
