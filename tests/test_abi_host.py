"""CPU tests of the C ABI as Python binds it: framedipt_amd/_lib.py derives its structs, signatures and constants from include/fdipt.h
through framedipt_amd/_header.py, and the host C compiler says whether they are the layout and the values the library was built with."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from framedipt_amd import _header, _lib

INCLUDE = os.path.join(ROOT, "include")
C_NAME = {t: n for n, t in reversed(list(_header.SCALARS.items()))}  # ctypes scalar -> a C spelling of it


def test_layout_and_macro_values_match_the_host_compiler(tmp_path):
    """A C program generated from the reader's output, compiled against include/fdipt.h: sizeof of every struct, offsetof and sizeof of
    every member and the value of every integer macro against the ctypes classes and the constants of _lib.  The program also takes
    each member through a pointer of the type the reader gave it (a void* where it says pointer), so a float read as an int32_t or a
    scalar read as a pointer stops the compilation."""
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    header = _lib._H
    lines = ["#include <stdio.h>", '#include "fdipt.h"', "int main(void) {"]
    for name, cls in header.structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines.append(f"  {{ static const {name} zero; const {name}* s = &zero;")
        for member, t in cls._fields_:
            lines.append(f'    printf("{name}.{member} %zu %zu\\n", offsetof({name}, {member}), sizeof(s->{member}));')
            typed = {C.c_void_p: f"const void* p = s->{member}", C.POINTER(C.c_void_p): f"void** p = s->{member}"}.get(t) or f"const {C_NAME[t]}* p = &s->{member}"
            lines.append(f"    {{ {typed}; (void)p; }}")
        lines.append("  }")
    lines += [f'  printf("FDIPT_{name} %lld\\n", (long long)(FDIPT_{name}));' for name in header.macros]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror=incompatible-pointer-types", "-Werror=int-conversion", "-I", INCLUDE,
                    str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {k: [int(x) for x in v.split()] for k, v in (line.split(" ", 1) for line in out.splitlines())}
    want = {}
    for name, cls in header.structs.items():
        assert cls is getattr(_lib, name[len("Fdipt"):])
        want[name] = [C.sizeof(cls)]
        want.update({f"{name}.{member}": [getattr(cls, member).offset, getattr(cls, member).size] for member, _ in cls._fields_})
    want.update({f"FDIPT_{name}": [getattr(_lib, name)] for name in header.macros})
    assert got == want
    assert len(header.structs) >= 6 and len(header.macros) >= 26 and len(want) >= 6 + 173 + 26


def test_every_prototype_is_bound_and_exported():
    """SIGNATURES holds the prototypes of the header and nothing else - found here by a plain search for ``fdipt_<name>(`` at the start of
    a statement, not by the reader - every parameter has a name and a type, and the built library exports every entry."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, "fdipt.h")).read(), flags=re.S)
    declared = re.findall(r"(?:^|[;}])\s*(?:const char\*|\w+)\s+(fdipt_\w+)\s*\(", text)
    assert len(declared) >= 62 and len(set(declared)) == len(declared)
    assert set(declared) == set(_lib.SIGNATURES) == set(_lib._H.functions)
    for name, (restype, argtypes, names) in _lib._H.functions.items():
        assert _lib.SIGNATURES[name] == (restype, argtypes) and len(names) == len(argtypes) == len(set(names)), name
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in declared:
            assert hasattr(lib, name), name


def test_type_rules_of_the_reader():
    """One entry per rule: scalars by value, device pointers as void*, the stream, struct pointers, ``_host`` scalar pointers with their
    pointee type, ``void**``, the ``const char*`` return - and a 22-argument positional signature, letter by letter."""
    s, i, d, f, p = _lib.SIGNATURES, C.c_int, C.c_double, C.c_float, C.c_void_p
    assert s["fdipt_se3_reverse_step"] == (i, [i, i] + [p] * 6 + [d] * 3 + [i] * 3 + [d] * 5 + [p] * 3)
    assert s["fdipt_r3_trans_score"] == (i, [i, i, p, p, p, f, f, f, p, p, p])
    assert s["fdipt_param_offset"] == (C.c_int64, [C.POINTER(_lib.Dims), i])
    assert s["fdipt_score_forward"] == (i, [C.POINTER(_lib.Dims), p, p, p, C.POINTER(_lib.ForwardArgs), p, C.c_size_t, p])
    assert s["fdipt_selftest_mfma"] == (i, [i, C.POINTER(d)]) and s["fdipt_violation_constants"] == (i, [C.POINTER(d)])
    assert s["fdipt_event_elapsed_ms"] == (i, [p, p, C.POINTER(f)]) and s["fdipt_kernel_class_bounds"] == (i, [C.POINTER(C.c_int32), i])
    assert s["fdipt_event_create"] == (i, [C.POINTER(p)]) and s["fdipt_version"] == (C.c_char_p, [])
    fields = dict(_lib.ForwardArgs._fields_)
    assert fields["ev_start"] is C.POINTER(p) and fields["clock_out"] is p and fields["reserve_cus"] is C.c_int32
    assert dict(_lib.SelectArgs._fields_)["group_start_host"] is p  # the pointee rule is for parameters, not members


STRUCT = "typedef struct FdiptX { int32_t n; %s; } FdiptX;"


@pytest.mark.parametrize("snippet,quoted", [
    (STRUCT % "long double x", "long double x"),                                   # an unknown type
    (STRUCT % "float v[3]", "float v[3]"),                                         # an array member
    (STRUCT % "int32_t flag : 1", "int32_t flag : 1"),                             # a bit-field
    (STRUCT % "float *a, *b", "float *a, *b"),                                     # another declarator style
    ("typedef struct FdiptY { int32_t n; } FdiptY; " + STRUCT % "FdiptY y", "FdiptY y"),   # a struct by value
    ("int fdipt_f(int, float* x);", "'int'"),                                      # an unnamed parameter
    ("int fdipt_f(int (*callback)(int), void* p);", "int (*callback)(int)"),       # a function pointer
    ("void fdipt_f(int n);", "void fdipt_f"),                                      # a return type the table does not have
    ("#define FDIPT_SCALE 1.5", "FDIPT_SCALE 1.5"),                                # FDIPT_ macros that are no integers
    ("#define FDIPT_MAX(a, b) ((a) > (b) ? (a) : (b))", "FDIPT_MAX"),
    ("#ifndef FDIPT_H\n#define FDIPT_H\n#define FDIPT_OTHER_H\n#endif", "FDIPT_OTHER_H"),   # only the include guard may be empty
])
def test_reader_refuses_what_it_does_not_understand(snippet, quoted):
    with pytest.raises(_header.HeaderError) as err:
        _header.parse(snippet)
    assert quoted in str(err.value)


def test_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "fdipt.h"))
    with pytest.raises(_lib.FdiptError, match=re.escape(str(tmp_path / "include" / "fdipt.h"))):
        _lib._read_header()


def test_numbers_of_the_abi_are_pinned():
    """The values callers and stored results depend on: renumbering the header fails here."""
    flags = {k: v for k, v in vars(_lib).items() if k.startswith("KF_") and k != "KF_ALL"}
    assert len(flags) >= 9 and _lib.KF_ALL == 2015 == sum(flags.values()) and 32 not in flags.values()
    assert (_lib.KF_ET3, _lib.KF_GENERIC_PAIR, _lib.KF_GENERIC_ATTN, _lib.KF_UNFUSED_NODE, _lib.KF_UNFOLDED, _lib.KF_NO_MERGE, _lib.KF_ROWS32,
            _lib.KF_PASS_Z, _lib.KF_POINTS_LAUNCH, _lib.KF_STREAM_ATTN) == (1, 2, 4, 8, 16, 64, 128, 256, 512, 1024)
    assert (_lib.PREC_F32, _lib.PREC_BF16, _lib.PREC_F16, _lib.PREC_F16X) == (0, 1, 2, 3)
    assert _lib.SELECT_MAX_SAMPLES == 64 and (_lib.SELECT_ZERO_DISTANCE, _lib.SELECT_SKIPPED) == (1, 2)
    assert (_lib.EVAL_NAN_DIHEDRAL, _lib.EVAL_DEGENERATE_ALIGNMENT, _lib.EVAL_SKIPPED) == (1, 2, 4)
    assert _lib.VIOLATION_CONSTANTS == 61
    assert (_lib.OK, _lib.EINVAL, _lib.ELAUNCH, _lib.ESIZE) == (0, -1, -2, -3) and sorted(_lib._ERR) == [-3, -2, -1]
